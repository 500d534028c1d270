"""csrc/m521_device.hpp and csrc/chacha_device.hpp, operation by operation,
on the device.

lib/libdn_opcheck.so (csrc/opcheck.hip over csrc/opcheck_ops.hpp) runs case i
of a section of tests/device_ops.py in lane i, 256-thread workgroups; every
result is compared with the Python references there, bit for bit — the same
sections and the same references as test_device_ops_host.py, which runs the
headers on the host against stand-ins for alignbit, the buffer loads and
stores, subc and __ballot.  This run is what shows that the stand-ins mean
what the hardware does, and it pins the device compiler's code for the paths
no kernel input reaches (prng_retry, long carry ripples, every odd divisor).

Each test is one launch and a read-back.
"""
import ctypes
import os
import time

import numpy as np
import pytest
import torch

import device_ops as do

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "delta-node_amd", "lib", "libdn_opcheck.so")


@pytest.fixture(scope="module")
def opcheck():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    assert os.path.isfile(LIB), f"{LIB} is missing: build it (make -C delta-node_amd)"
    lib = ctypes.CDLL(LIB)
    lib.dn_opcheck_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.dn_opcheck_run.restype = ctypes.c_int
    for name, (op, iw, ow) in do.OPS.items():
        assert (lib.dn_opcheck_in_words(op), lib.dn_opcheck_out_words(op)) == (iw, ow), name
    assert lib.dn_opcheck_in_words(len(do.OPS)) == 0
    dev = torch.device("cuda", torch.cuda.current_device())

    def run(sec: do.Section) -> bytes:
        n = len(sec.cases)
        t0 = time.perf_counter()
        tin = torch.from_numpy(np.frombuffer(sec.records, dtype=np.uint8).copy()).to(dev)
        rec = np.frombuffer(do.fill(4 * sec.ow), dtype=np.uint8)
        tout = torch.from_numpy(rec.copy()).to(dev).repeat(n)
        assert tin.numel() == 4 * sec.iw * n and tout.numel() == 4 * sec.ow * n
        rc = lib.dn_opcheck_run(sec.op_id, tin.data_ptr(), tout.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, f"dn_opcheck_run rc={rc}"
        torch.cuda.synchronize()
        out = tout.cpu().numpy().tobytes()
        print(f"{sec.name}: {n} lanes, launch and read-back {time.perf_counter() - t0:.3f} s")
        return out

    return run


@pytest.mark.parametrize("name", [n for n in do.section_names() if not n.startswith("store_reduced")])
def test_device_op(opcheck, name):
    t0 = time.perf_counter()
    sec = do.section(name)
    sec.check(opcheck(sec))
    print(f"{name}: whole test {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("op", ["store_reduced", "store_reduced_at"])
def test_device_store_reduced_by_wave_kind(opcheck, op):
    """Lanes ordered so that whole waves are ordinary, all rare, or rare in
    lane 0, lane 63 or one middle lane only: D is reduced in place exactly
    where a lane of the same wave is rare, and the stored value is D mod p
    either way."""
    t0 = time.perf_counter()
    sec = do.section(op)
    lay = do.store_reduced_layout()
    c = do.wave_census(lay)
    assert c["none"] >= 2 and c["all"] >= 2 and c["only0"] == 1 and c["only63"] == 1 and c["only_mid"] == 1, c
    sec.check(opcheck(sec), wave_rare=do.wave_rare_of(lay))
    print(f"{op}: whole test {time.perf_counter() - t0:.2f} s")
