# (run by tests/test_gpu_nmf_batch.py in a fresh interpreter) nmf_batch as the FIRST device call of a process that never imports torch:
# no context exists, nothing has initialised the GPU; PMX_DEVICE names the GPU.  Prints a digest of the results.
import hashlib, os, sys
os.environ["PMX_TORCH_PRELOAD"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import proxmin_amd as pm
from oracle import nmf_oracle as orc
shapes = [(33, 47, 3), (40, 257, 9), (8, 40, 8)]
Ys, As, Ss = zip(*[orc.synthetic_problem(*s, dtype=np.float32, seed=1234) for s in shapes])
try:
    res = pm.nmf_batch(Ys, As, Ss, max_iter=5, e_rel=1e-9)
except pm._lib.PmxError as exc:
    print("PmxError:", exc)
    sys.exit(3)
assert "torch" not in sys.modules
h = hashlib.sha256()
for x in list(As) + list(Ss) + [res.steps, res.iterations, res.converged]:
    h.update(np.ascontiguousarray(x).tobytes())
print("digest", h.hexdigest())
