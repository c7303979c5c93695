"""GPU: which K1 a context runs, pinned (pmx_api.hip: select_k1, k1_instance; include/pmx.h: pmx_k1_info).

Every mode x K1's K x an aligned, a ragged (framed) and a small shape (chained and re-framed ones at K = 32, 64, 128), with and without weights, plus the environment switches
that steer the choice: the whole k1_info() dict before the first launch, after one gradient pass, with W set and cleared again,
after Y handed over with an odd pitch (the v8 -> v7 fall-back) and after the range fall-back.  The table was recorded before
the kernel choice was folded into one kind per context; any change in it is a change of behaviour."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = {"aligned": (1024, 2048), "ragged": (1000, 1500), "small": (200, 300),
          "chained": (4096, 4096), "reframed": (16383, 4097)}      # (gA summed along chains; the frame search for a chained frame)
MODES = ("f32", "bf16x3", "f16x2", "f16x2r")
KS = (8, 16, 32, 48, 64, 100, 128)

CASES = ([(m, k, s, w, "") for m in MODES for k in KS for s in ("aligned", "ragged", "small") for w in (False, True)] +
         [(m, k, "ragged", False, "PMX_FRAME=0") for m in MODES for k in KS] +
         [(m, k, "aligned", False, "PMX_F16_R3=1") for m in ("f16x2", "f16x2r") for k in KS] +
         [(m, 64, "aligned", False, e) for m in ("bf16x3", "f16x2", "f16x2r") for e in ("PMX_K1_CHAIN=0", "PMX_K1_VARIANT=0", "PMX_K1_VARIANT=1")] +
         [(m, k, s, w, "") for m in MODES for k in (32, 64, 128) for s in ("chained", "reframed") for w in (False, True) if not (w and s == "reframed")] +
         [(m, k, "chained", False, e) for m in MODES for k in (64, 128) for e in ("PMX_K1_CHAIN=0", "PMX_K1_CHAIN=4")] +
         [(m, k, "aligned", False, "odd_ld_Y") for m in ("f16x2", "f16x2r") for k in (64, 128)] +
         [(m, k, "aligned", False, "far_start") for m in ("f16x2", "f16x2r") for k in (32, 64, 128)])


def case_id(case):
    mode, K, shape, w, extra = case
    return "%s-K%d-%s%s%s" % (mode, K, shape, "-W" if w else "", "-" + extra if extra else "")


def _info(dev):
    d = dev.k1_info()
    d["frame"] = list(d["frame"])
    return d


def observe(case, monkeypatch):
    """the k1_info() dicts of one case, in the order of the steps taken (a step the context refuses: its error class name)"""
    import torch
    from proxmin_amd import engine
    mode, K, shape, w, extra = case
    M, N = SHAPES[shape]
    if "=" in extra:
        monkeypatch.setenv(*extra.split("="))
    rng = np.random.default_rng(M + N + K)
    A = rng.uniform(0.1, 1.0, (M, K)).astype(np.float32)
    S = rng.uniform(0.1, 1.0, (K, N)).astype(np.float32)
    Y = (A @ S + rng.uniform(0.0, 0.1, (M, N))).astype(np.float32)
    if extra == "far_start":
        A, S = (A * 3e3).astype(np.float32), (S * 1e4).astype(np.float32)
    seen = []
    with engine.DeviceNMF(M, N, K, mode=mode) as dev:
        seen.append(_info(dev))
        if extra == "odd_ld_Y":
            Yt = torch.zeros((M, N + 1), dtype=torch.float32, device="cuda")
            Yt[:, :N] = torch.from_numpy(Y)
            dev.set_Y_device(Yt.data_ptr(), ld=N + 1, copy=False, keepalive=Yt)
        else:
            dev.set_Y(Y)
        dev.set_factors(A, S)
        seen.append(_info(dev))
        dev.grad()
        seen.append(_info(dev))
        if extra == "odd_ld_Y":
            dev.set_Y(Y)
            dev.grad()
            seen.append(_info(dev))
        if w:
            try:
                dev.set_W(rng.uniform(0.5, 2.0, (M, N)).astype(np.float32))
                dev.grad()
                seen.append(_info(dev))
            except Exception as e:       # (a kind that takes no weights refuses them)
                seen.append(type(e).__name__)
            dev.set_W(None)
            seen.append(_info(dev))
            dev.grad()
            seen.append(_info(dev))
    return seen


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_k1_selection_is_pinned(case, monkeypatch):
    import __graft_entry__ as g
    g.build()
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k1_select.json")) as f:
        want = json.load(f)[case_id(case)]
    assert observe(case, monkeypatch) == want
