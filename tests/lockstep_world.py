"""W ranks of a row-sharded solve in ONE process, driven in lockstep (a test helper, not a conftest).

`pmx_set_world(ctx, rank, world, M_global)` describes a rank completely and the collective is the caller's, so W contexts
whose phase calls are issued rank after rank, with the collective done as a plain sum over their comm buffers, execute the
kernels a W-GPU run executes -- every rank number, unequal shards, more than two addends -- without W processes.  Only one
context's kernels are ever in flight.

The drivers of proxmin_amd/distributed.py (ShardedAdaproxDriver, ShardedLoop) run UNMODIFIED: they are handed

  LockstepEngine  one engine-shaped object: phase / more_subs / tail_fused fan out over the ranks' engines (each rank's call is
                  synchronised before the next rank starts), chain_status reads every rank and insists that they agree;
                  comm / comm_out / st_full / st_iterate are `PerRank` handles (one tensor per rank);
  LockstepDist    one torch.distributed-shaped object whose three collectives act on those handles.

Both are generic over the engines: tests/test_lockstep_world_cpu.py drives the NumPy stand-in engines of
tests/test_distributed_cpu.py through them (no GPU), tests/test_gpu_sharded_lockstep.py the product's ShardEngine, which
`LockstepWorld` opens -- one DeviceNMF per entry of `row_ranges`, each on a private stream."""
import ctypes as C

import numpy as np
import torch

from proxmin_amd.distributed import HALT_PEER, HALT_RETRY, ShardedAdaproxDriver, ShardedLoop

# a halt that the protocol repairs by itself: the rank whose K1 refused or faulted reads HALT_RETRY, its peers -- stopped
# through the collective halt flag before the same iteration's update -- read HALT_PEER; the drivers go on from it_done on both
_REPAIRED = (HALT_RETRY, HALT_PEER)


class PerRank:
    """One tensor per rank where the drivers expect one tensor; as much of a tensor as they use on the way to a collective."""

    def __init__(self, tensors):
        self.tensors = list(tensors)

    def numel(self):
        n = {t.numel() for t in self.tensors}
        assert len(n) == 1, "the ranks' buffers differ in size: %r" % sorted(n)
        return n.pop()

    def view(self, *shape):
        return PerRank(t.view(*shape) for t in self.tensors)

    def clone(self):
        return PerRank(t.clone() for t in self.tensors)

    def __getitem__(self, key):
        return PerRank(t[key] for t in self.tensors)

    @property
    def device(self):
        return self.tensors[0].device


def _device_sync(tensors):
    if tensors[0].is_cuda:
        torch.cuda.synchronize()


class LockstepDist:
    """torch.distributed's three collectives of the sharded drivers over PerRank handles, as plain sums and copies."""

    class ReduceOp:
        SUM = None

    def __init__(self, world):
        self.world = int(world)
        self.after = []              # callables (name, handles...) run behind every collective: the tests' look into the buffers

    def get_rank(self, group=None):
        return 0                     # (all_gather_chunks slices "its" chunk with this; the gather below ignores that slice)

    def get_world_size(self, group=None):
        return self.world

    def _done(self, name, *handles):
        _device_sync(handles[0].tensors)
        for fn in self.after:
            fn(name, *handles)

    def all_reduce(self, t, op=None, group=None):
        """every rank's buffer <- the sum over the ranks, added in rank order in the buffers' own precision"""
        assert len(t.tensors) == self.world
        _device_sync(t.tensors)
        total = t.tensors[0].clone()
        for q in range(1, self.world):
            total += t.tensors[q]
        for x in t.tensors:
            x.copy_(total)
        self._done("all_reduce", t)

    def reduce_scatter_tensor(self, out, inp, op=None, group=None):
        """rank q's `out` <- the sum over the ranks of chunk q of their `inp`"""
        assert len(out.tensors) == len(inp.tensors) == self.world
        n = out.numel()
        assert inp.numel() == n * self.world
        _device_sync(inp.tensors)
        for q in range(self.world):
            total = inp.tensors[0][q * n:(q + 1) * n].clone()
            for r in range(1, self.world):
                total += inp.tensors[r][q * n:(q + 1) * n]
            out.tensors[q].copy_(total)
        self._done("reduce_scatter", out, inp)

    def all_gather_into_tensor(self, out, inp=None, group=None):
        """rank q's own piece q of `out` to every rank's `out`, in each rank's own buffer"""
        assert len(out.tensors) == self.world
        n = out.numel() // self.world
        assert n * self.world == out.numel()
        _device_sync(out.tensors)
        pieces = [out.tensors[q][q * n:(q + 1) * n].clone() for q in range(self.world)]
        for r in range(self.world):
            for q in range(self.world):
                if q != r:
                    out.tensors[r][q * n:(q + 1) * n].copy_(pieces[q])
        self._done("all_gather", out)


class LockstepEngine:
    """The ranks' engines behind the interface of ONE engine (what _ShardedDriver is written against)."""

    def __init__(self, engines):
        self.engines = list(engines)
        split = {bool(getattr(e, "s_split", False)) for e in self.engines}
        assert len(split) == 1
        self.s_split = split.pop()
        self.status_log = []         # every chain_status reading: [(halted, reason, it_done, tau) per rank]

    def _fan(self, name, *args):
        out = []
        for e in self.engines:
            out.append(getattr(e, name)(*args))
            dev = getattr(e, "dev", None)
            if dev is not None:
                dev.sync()           # this rank's kernels have finished before the next rank's start
        return out

    def phase(self, *args):
        self._fan("phase", *args)

    def more_subs(self, t0, n):
        self._fan("more_subs", t0, n)

    def tail_fused(self):
        return all(bool(e.tail_fused()) if hasattr(e, "tail_fused") else False for e in self.engines)

    def chain_status(self):
        st = self._fan("chain_status")
        self.status_log.append(st)

        def key(s):
            return (s[0], HALT_RETRY if s[0] and s[1] in _REPAIRED else s[1], s[2])
        assert len({key(s) for s in st}) == 1, "the ranks disagree about (halted, reason, it_done): %r" % (st,)
        tau = tuple(max(s[3][j] for s in st) for j in range(2))
        return st[0][0], st[0][1], st[0][2], tau

    def _handle(self, name):
        ts = [getattr(e, name, None) for e in self.engines]
        if all(t is None for t in ts):
            return None
        assert all(t is not None for t in ts), "%s is bound on some ranks only" % name
        return PerRank(ts)

    comm = property(lambda self: self._handle("comm"))
    comm_out = property(lambda self: self._handle("comm_out"))

    @property
    def st_full(self):
        return self._handle("st_full")

    @property
    def st_iterate(self):
        """FISTA under S-split: bind_eval_buffer has swapped the two buffers on every rank (the evaluation point is gathered every
        iteration, the iterate once per run); they are two buffers, told apart by their addresses, rank by rank"""
        h = self._handle("st_iterate")
        if h is not None:
            for it_, full in zip(h.tensors, self.st_full.tensors):
                assert it_.data_ptr() != full.data_ptr()
        return h


class LockstepWorld:
    """`len(row_ranges)` contexts of the HIP library for one problem Y ~ A S: rank r holds rows row_ranges[r] of Y and A0 and all
    of S0, is wrapped in the product's ShardEngine and begun with `algorithm` ("adaprox" | "pgm" | "bsdmm") and `solver_kw` (the
    keywords of DeviceNMF.*_begin; prox_A / prox_S are operators of proxmin_amd.operators, default prox_plus; bsdmm: proxs_g as
    for nmf()).  `engine` and `dist` go to the product's drivers (`driver()` builds the one the algorithm's front end builds)."""

    def __init__(self, Y, A0, S0, row_ranges, algorithm, mode, s_split=False, prox_A=None, prox_S=None, proxs_g=None, **solver_kw):
        from proxmin_amd import distributed as pdist, operators
        from proxmin_amd.engine import DeviceNMF
        self.row_ranges = [(int(a), int(b)) for a, b in row_ranges]
        self.algorithm, self.mode, self.solver_kw = algorithm, mode, dict(solver_kw)
        M, K = A0.shape
        N = S0.shape[1]
        assert self.row_ranges[0][0] == 0 and self.row_ranges[-1][1] == M
        assert all(a[1] == b[0] for a, b in zip(self.row_ranges, self.row_ranges[1:]))
        W = len(self.row_ranges)
        self.devs, self.streams, self.shards = [], [], []
        self.seqs = [operators.device_proxseq(operators.prox_plus if q is None else q, j) for j, q in enumerate((prox_A, prox_S))]
        try:
            for r, (r0, r1) in enumerate(self.row_ranges):
                stream = torch.cuda.Stream()
                self.streams.append(stream)
                dev = DeviceNMF(r1 - r0, N, K, mode=mode, stream=stream.cuda_stream)
                self.devs.append(dev)
                dev.set_Y(np.ascontiguousarray(Y[r0:r1]))
                dev.set_factors(np.ascontiguousarray(A0[r0:r1]), S0)
                eng = pdist.ShardEngine(dev, W, r, M, algorithm, s_split)
                self.shards.append(eng)
                if algorithm == "adaprox":
                    dev.adaprox_begin(self.seqs, **solver_kw)
                elif algorithm == "pgm":
                    dev.pgm_begin(self.seqs, **solver_kw)
                    eng.bind_eval_buffer()
                else:
                    seq_g = [None if g is None else [operators.device_proxseq(q, j) for q in g] for j, g in enumerate(proxs_g or [None, None])]
                    dev.bsdmm_begin(self.seqs, seq_g, **solver_kw)
                dev.sync()
            torch.cuda.synchronize()     # (the comm buffers were zeroed on torch's stream, the kernels run on the contexts')
        except BaseException:
            self.close()
            raise
        self.engine = LockstepEngine(self.shards)
        self.dist = LockstepDist(W)

    def driver(self, chunk=None):
        if self.algorithm == "adaprox":
            kw = self.solver_kw
            return ShardedAdaproxDriver(self.engine, None, kw.get("check_convergence", True), self.seqs[0].n > 0 or self.seqs[1].n > 0,
                                        kw.get("prox_max_iter", 1000), chunk=chunk, dist_module=self.dist)
        return ShardedLoop(self.engine, None, deferred_test=self.algorithm == "pgm", dist_module=self.dist, **({} if chunk is None else {"chunk": chunk}))

    def run(self, max_iter, b1=0.9, chunk=None):
        """the product's loop over the lockstep engine -> (iterations, the driver)"""
        drv = self.driver(chunk)
        n = drv.run(max_iter, np.full(max_iter, b1, dtype=np.float64)) if self.algorithm == "adaprox" else drv.run(max_iter)
        return n, drv

    def factors(self):
        """[(A rows, S) of rank r]"""
        return [dev.get_factors() for dev in self.devs]

    def results(self):
        """pmx_iter_result of every rank"""
        from proxmin_amd import _lib
        out = []
        for dev in self.devs:
            r = _lib.Result()
            _lib.check(dev.lib.pmx_iter_result(dev.h, C.byref(r)))
            out.append(r)
        return out

    def k1_infos(self):
        return [dev.k1_info() for dev in self.devs]

    def close(self):
        err = None
        for dev in self.devs:
            try:
                dev.close()
            except Exception as exc:     # noqa: BLE001 -- every context is destroyed, the first failure is reported
                err = err or exc
        self.devs = []
        if err is not None:
            raise err

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
