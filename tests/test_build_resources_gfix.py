"""Register-allocation guard for the K1 instances that carry the K x K correction (k_grad_f16_v8<.., HH, RS, .., GF>), CPU-side like
tests/test_build_resources.py: hipcc cross-compiles gfx950 without a GPU.

K1's waves hold all 256 registers a wave can have at two waves per SIMD; the three stages of the correction run before and behind K1's
loops and must not take registers from them.  The pins are test_build_resources.py's own for the <.., HH, RS> instances (4 spilled VGPRs
chained, 2 with one gA slab per column region); scratch is bounded by the instance without the ride from the same build."""
import os
import re
import subprocess
import tempfile

import pytest

import __graft_entry__ as g

# <PROF=0, HASW=0, CHAIN, LOSS=0, R3=0, HH=1, RS=1, ONLYS=0, Y16, GF>
NAME = "_Z13k_grad_f16_v8ILb0ELb0ELb%dELb0ELb0ELb1ELb1ELb0ELb%dELb%dEEv10GradV4Args"
SPILL_PIN = {1: 4, 0: 2}     # by CHAIN


@pytest.fixture(scope="module")
def usage():
    try:
        hipcc = g._hipcc()
    except RuntimeError:
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "--cuda-device-only", "-c",
               "-Rpass-analysis=kernel-resource-usage", os.path.join(g.CSRC, "pmx_api.hip"), "-o", os.path.join(tmp, "pmx.o")]
        r = subprocess.run(cmd, cwd=g.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
        m = re.search(r"(VGPRs Spill|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            out[cur][m.group(1)] = int(m.group(2))
    assert out, "no resource-usage remarks in the compiler output"
    return out


@pytest.mark.parametrize("chain", [1, 0], ids=["chained", "slabs"])
@pytest.mark.parametrize("y16", [1, 0], ids=["y16", "y8"])
def test_instances_that_carry_the_correction(usage, chain, y16):
    ride, plain = NAME % (chain, y16, 1), NAME % (chain, y16, 0)
    assert ride in usage, "kernel %s not found in the build" % ride
    assert plain in usage, "kernel %s not found in the build" % plain
    r, p = usage[ride], usage[plain]
    print(ride, r, "without the ride:", p)
    assert r["VGPRs Spill"] <= SPILL_PIN[chain], (r, p)
    assert r["ScratchSize [bytes/lane]"] <= p["ScratchSize [bytes/lane]"], (r, p)
    assert r["Occupancy [waves/SIMD]"] == p["Occupancy [waves/SIMD]"] == 2, (r, p)


def test_the_flag_is_accepted_with_both_gradients_only(usage):
    """<.., GF> exists for the role-split two-gradient pass alone: no loss-only, row-split or gSt-only instance carries the correction"""
    rides = [k for k in usage if re.match(r"_Z13k_grad_f16_v8I(Lb[01]E){9}Lb1EEv", k)]
    assert sorted(rides) == sorted(NAME % (c, y, 1) for c in (0, 1) for y in (0, 1)), rides
