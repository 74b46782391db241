"""The parameter table the four network handles share (csrc/paramtable.h), without a GPU.

(a) Through the C ABI: the decoder, the denoiser and the point-cloud encoder refuse the same wrong calls with the same codes and
    name the tensor; nothing is allocated before the checks (a null pointer after a right shape is SURFD_ERR_ARG = -1, not
    SURFD_ERR_HIP = -3, on a host without a device); finalize names the first tensor that was not set.
(b) tools/paramtable_check.cpp: the table itself in a stand-alone program built with the host's address and undefined-behaviour
    sanitizers and run directly."""
import ctypes as C
import os
import subprocess

import pytest

from surfd_amd import _native as N
from surfd_amd import build as B
from test_abi_cpu import _unet_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        B.build_library()
    return N.lib()


def _create(lib, which):
    h = C.c_void_p()
    if which == "decoder":
        N.check(lib.surfd_decoder_create(63, 32, 512, 5, C.byref(h)))
    elif which == "unet":
        N.check(lib.surfd_unet_create(C.byref(_unet_cfg()), C.byref(h)))
    else:
        N.check(lib.surfd_dgcnn_create(32, 20, C.byref(h)))
    return h


def _table(lib, which, h):
    fn = getattr(lib, f"surfd_{which}_param_info")
    out = []
    for i in range(getattr(lib, f"surfd_{which}_num_params")(h)):
        key, shp, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        N.check(fn(h, i, C.byref(key), shp, C.byref(nd)))
        out.append((key.value, tuple(shp[:nd.value])))
    return out


@pytest.mark.parametrize("which", ["decoder", "unet", "dgcnn"])
def test_set_param_and_finalize_refusals(lib, which):
    h = _create(lib, which)
    set_param = getattr(lib, f"surfd_{which}_set_param")
    finalize = getattr(lib, f"surfd_{which}_finalize")
    info = getattr(lib, f"surfd_{which}_param_info")
    num = getattr(lib, f"surfd_{which}_num_params")(h)
    try:
        table = _table(lib, which, h)
        assert len(table) == num > 0
        key, shape = next((k, s) for k, s in table if not k.endswith(b"num_batches_tracked"))
        assert len(shape) >= 1
        dummy = C.c_void_p(256)                       # never read: every call below is refused before anything is copied

        assert set_param(h, b"no.such.tensor", dummy, N.shape_arr(shape), len(shape), None) == ERR_ARG
        assert b"no.such.tensor" in lib.surfd_last_error()

        assert set_param(h, key, dummy, N.shape_arr(shape + (1,)), len(shape) + 1, None) == ERR_ARG      # wrong rank
        assert key in lib.surfd_last_error() and b"rank" in lib.surfd_last_error()

        wrong = shape[:-1] + (shape[-1] + 1,)
        assert set_param(h, key, dummy, N.shape_arr(wrong), len(wrong), None) == ERR_ARG                 # one wrong dimension
        assert key in lib.surfd_last_error()

        # right shape, null pointer: refused as an argument error, so nothing was allocated before the checks
        assert set_param(h, key, None, N.shape_arr(shape), len(shape), None) == ERR_ARG
        assert key in lib.surfd_last_error()

        assert finalize(h, None) == ERR_STATE
        assert b"not set" in lib.surfd_last_error() and b"'" + key + b"'" in lib.surfd_last_error()

        if which != "unet":
            nbt = next(k for k, s in table if k.endswith(b"num_batches_tracked"))
            assert set_param(h, nbt, None, N.shape_arr(()), 0, None) == 0
            assert finalize(h, None) == ERR_STATE
            assert b"'" + key + b"'" in lib.surfd_last_error()

        k2, shp, nd = C.c_char_p(), (C.c_int64 * 4)(), C.c_int()
        assert info(h, -1, C.byref(k2), shp, C.byref(nd)) == ERR_ARG
        assert info(h, num, C.byref(k2), shp, C.byref(nd)) == ERR_ARG
    finally:
        getattr(lib, f"surfd_{which}_destroy")(h)


def test_table_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "paramtable_check")
    src = os.path.join(ROOT, "tools", "paramtable_check.cpp")
    assert '#include "../surfd_amd/csrc/paramtable.h"' in open(src).read()
    r = subprocess.run([B._hipcc(), "-std=c++17", "-O1", "-g", "-x", "hip", "--cuda-host-only", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "paramtable_check: OK" in r.stdout
