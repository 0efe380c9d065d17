"""The C ABI library loads and exports every symbol include/lakeside_gpu.h declares (CPU; no compute)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lakeside_gpu.h")


def declared_symbols():
    text = open(HEADER).read()
    return sorted(set(re.findall(r"\b(lk_[a-z_]+)\s*\(", text)))


def test_header_declares_the_boundary():
    syms = declared_symbols()
    for s in ["lk_engine_create", "lk_eval_pushdown", "lk_result_tag_value", "lk_last_error", "lk_comm_init",
              "lk_eval_pushdown_dist", "lk_segment_put"]:
        assert s in syms


def test_library_exports_every_declared_symbol():
    from lakeside_amd import _lib
    L = _lib.lib()
    for s in declared_symbols():
        assert hasattr(L, s), s
    bound = {name for name, _, _ in _lib.SIGNATURES}
    assert set(declared_symbols()) == bound, "ctypes signature table out of sync with the header"


def test_library_is_gfx950_code_object():
    lib = os.path.join(ROOT, "lakeside_amd", "liblakeside_gpu.so")
    data = open(lib, "rb").read()
    assert b"amdgcn-amd-amdhsa--gfx950" in data          # the embedded code object targets gfx950 only
    assert b"--gfx942" not in data and b"--gfx90a" not in data


def test_engine_create_without_gpu_fails_loudly():
    """No silent CPU fallback: creating an engine with no HIP device is an error.  Runs in a child process that sees
    no GPU (any GPU of this host is hidden from it), so the test process itself never initialises a HIP runtime
    here: torch ships its own copy of the runtime, and once that one is initialised in a process the library's
    own cannot find the device any more."""
    code = ("import ctypes\n"
            "from lakeside_amd import _lib\n"
            "import torch  # noqa: F401  (only to mirror the GPU-box environment; device count via HIP below)\n"
            "h = ctypes.c_void_p()\n"
            "rc = _lib.lib().lk_engine_create(b'{}', ctypes.byref(h))\n"
            "assert rc == _lib.LK_ERR_DEVICE, rc\n"
            "assert b'device' in _lib.lib().lk_last_error().lower()\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


def test_bad_arguments_are_status_codes():
    from lakeside_amd import _lib
    L = _lib.lib()
    assert L.lk_eval_pushdown(None, b"{}", None, 0, 10, 1, None) == _lib.LK_ERR_ARG
    assert L.lk_result_num_rows(None) == 0
    assert L.lk_result_tag_name(None, 0) is None
    assert L.lk_comm_init(None, None, 1, 0) == _lib.LK_ERR_ARG
