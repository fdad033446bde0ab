"""CPU tests of the C ABI: the library builds/loads and exports every symbol
include/d2mi.h declares (no compute calls without a GPU)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "d2mi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(d2mi_\w+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import torch  # noqa: F401  (binds the HIP runtime torch ships)
    from detectron2_tensorflow_amd import _C, _build
    _build.build()
    lib = ctypes.CDLL(_C.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 20
    missing = [s for s in syms if not hasattr(lib, s)]
    assert not missing, missing
    # and the ctypes table covers exactly the declared API
    assert sorted(_C.EXPORTED) == syms


def test_loader_sets_signatures_and_version():
    from detectron2_tensorflow_amd import _C
    from detectron2_tensorflow_amd import _build
    lib = _C.load()
    assert lib.d2mi_version() == 1
    assert _C.last_error() == ""
    # built from exactly this tree's sources (the loader refuses otherwise)
    assert lib.d2mi_source_hash().decode() == _build.source_hash()


def test_host_side_argument_errors_raise_without_gpu():
    """Argument validation happens on the host before any launch."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    rc = lib.d2mi_nms(None, None, None, 1, 10, 10, 1.5, None, None, None, 0, None)
    assert rc < 0 and "iou_threshold" in _C.last_error()
    rc = lib.d2mi_conv2d_nhwc(None, None, None, None, None, None, 1, 8, 8, 3, 16, 3, 3, 1, 1, 1,
                              0, None)
    assert rc < 0 and "multiple of 4" in _C.last_error()


def _short_workspace_calls(lib):
    """(name, queried size, call taking workspace_bytes) of ops whose host code
    reaches the workspace carve before any HIP call or pointer dereference."""
    ws = ctypes.c_void_p(256)  # non-null, never dereferenced: the carve is refused first
    return [
        ("nms", lib.d2mi_nms_workspace_size(3, 100),
         lambda n: lib.d2mi_nms(None, None, None, 3, 100, 10, 0.5, None, None, ws, n, None)),
        ("group_norm", lib.d2mi_group_norm_workspace_size(2, 8, 8, 32, 4),
         lambda n: lib.d2mi_group_norm_nhwc(None, 2, 8, 8, 32, 4, None, None, 1e-5, 0, 0, 0, None,
                                            ws, n, None)),
        ("fast_rcnn", lib.d2mi_fast_rcnn_workspace_size(2, 16, 3, 0.05, 10),
         lambda n: lib.d2mi_fast_rcnn_inference(None, None, None, None, None, 0, 2, 16, 3, 0, None,
                                                None, 4.135, 0.05, 0.5, 10, None, None, None,
                                                None, None, ws, n, None)),
        ("topk", lib.d2mi_topk_workspace_size(3, 65),
         lambda n: lib.d2mi_topk(None, None, None, 3, 1000, 65, 0, None, None, None, ws, n, None)),
        ("matrix_nms", lib.d2mi_matrix_nms_workspace_size(65),
         lambda n: lib.d2mi_matrix_nms(None, None, None, None, 65, 64, 0, 2.0, None, ws, n, None)),
        ("solo_finalize", lib.d2mi_solo_finalize_workspace_size(2, 5, 65),
         lambda n: lib.d2mi_solo_finalize(None, None, None, None, 2, 4, 8, 8, 0.05, 5, 0.5, 65, 16,
                                          None, None, None, None, None, ws, n, None)),
    ]


def test_workspace_one_byte_short_is_refused_without_gpu():
    """Every op lays its workspace out with the function its *_workspace_size
    runs: one byte less than the queried size is refused on the host."""
    from detectron2_tensorflow_amd import _C
    lib = _C.load()
    for name, size, call in _short_workspace_calls(lib):
        assert size > 1, name
        rc = call(size - 1)
        msg = _C.last_error()
        assert rc < 0 and "too small" in msg and f"{size - 1} < {size}" in msg, (name, rc, msg)


def test_parsed_signatures_match_the_header():
    """The ctypes table is parsed from include/d2mi.h; one literal entry per type class."""
    from detectron2_tensorflow_amd import _C
    c = ctypes
    P, I, F, Z = c.c_void_p, c.c_int, c.c_float, c.c_size_t
    want = {
        "d2mi_nms": (I, [P, P, P, I, I, I, F, P, P, P, Z, P]),
        "d2mi_subsample": (I, [P, I, I, c.c_longlong, I, I, P, P, P, P, P, I, P, Z, P]),
        "d2mi_split_bf16x3": (I, [P, c.c_int64, P, P]),
        "d2mi_source_hash": (c.c_char_p, []),
        "d2mi_roi_align_bwd_workspace_size": (Z, [P, I, I, I, I, I, I]),
        "d2mi_error_word_dev": (P, []),
        "d2mi_set_tuning": (I, [c.c_char_p, I]),
    }
    sigs = _C.parse_header(open(os.path.join(ROOT, "include", "d2mi.h")).read())
    assert tuple(sigs) == _C.EXPORTED
    lib = _C.load()
    for name, (res, args) in want.items():
        assert sigs[name][0] is res and len(sigs[name][1]) == len(args), name
        assert all(a is b for a, b in zip(sigs[name][1], args)), name
        fn = getattr(lib, name)  # and load() put them on the functions
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_parser_refuses_a_type_it_does_not_know():
    import pytest
    from detectron2_tensorflow_amd import _C
    ok = "int d2mi_a(const float* x, int n);\nsize_t d2mi_b(void);\n"
    assert _C.parse_header(ok) == {"d2mi_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
                                   "d2mi_b": (ctypes.c_size_t, [])}
    for bad in ("int d2mi_c(double x);", "int d2mi_c(unsigned n);", "short d2mi_c(int n);",
                "int d2mi_c(my_handle_t h);", "int d2mi_c(int);"):
        with pytest.raises(TypeError):
            _C.parse_header(ok + bad)


TUNING_DEFAULTS = {
    "conv_epi": 1, "wgrad_ws1": 6, "wgrad_xcd": 1, "conv_xcd": 1, "conv_ws_mink": 16,
    "roi_pix_grid": 8192, "conv_stream": 8192, "retina_fused": 1, "rpn_merge": 1, "nms_scan": 1,
    "roi_heavy": 16, "rpn_compact": 1, "conv_stream_nt": 2, "conv_nt": 0, "conv_tail_mink": 8,
    "sgd_rev": 0, "retina_rank": 0, "solo_mfma": 2, "retina_var": 12018, "conv_split_slots": 0,
    "conv_tail": 1, "wgrad_occ3_min_p": 65536, "wgrad_slots": 0, "wgrad_minch": 16,
    "wgrad_maxsplit": 128, "wgrad_prio": 1, "topk_floor": 1,
}
# knobs fixed at their defaults and removed: unknown keys now
RETIRED_KNOBS = ("conv_ws", "roi_fwd", "wgrad_ws", "wgrad_inc", "roi_bwd_rec", "conv_ws_mintiles",
                 "conv_occ", "wgrad_occ", "roi_bwd_ppw")

_TUNING_CHILD = """
import json, sys
from detectron2_tensorflow_amd import _C
from detectron2_tensorflow_amd.layers import ops
out = {k: ops.get_tuning(k) for k in json.loads(sys.argv[1])}
out["<unknown get>"] = _C.lib().d2mi_get_tuning(b"no_such_knob")
try:
    ops.set_tuning("no_such_knob", 1)
    out["<unknown set>"] = "accepted"
except _C.D2MIError as e:
    out["<unknown set>"] = str(e)
retired = {}
for k in json.loads(sys.argv[2]):
    try:
        ops.set_tuning(k, 1)
        err = "accepted"
    except _C.D2MIError as e:
        err = str(e)
    retired[k] = [_C.lib().d2mi_get_tuning(k.encode()), err]
out["<retired>"] = retired
print(json.dumps(out))
"""


def _tuning_in_child(extra_env):
    """get_tuning of every knob in a fresh process whose only D2MI_* variables are extra_env."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith("D2MI_")}
    env.update(extra_env, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _TUNING_CHILD, json.dumps(list(TUNING_DEFAULTS)),
                        json.dumps(list(RETIRED_KNOBS))],
                       env=env, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_tuning_defaults_and_environment_without_gpu():
    """The 27 knobs' defaults, their D2MI_<KEY> environment variables, unknown keys, and the
    retired knobs among them."""
    from detectron2_tensorflow_amd import _build
    _build.build()
    got = _tuning_in_child({})
    assert got.pop("<unknown get>") == -2 ** 31
    assert "unknown tuning key" in got.pop("<unknown set>")
    retired = got.pop("<retired>")
    assert sorted(retired) == sorted(RETIRED_KNOBS)
    for k, (value, err) in retired.items():
        assert value == -2 ** 31 and "unknown tuning key" in err, k
    assert got == TUNING_DEFAULTS and len(got) == 27
    # (D2MI_CONV_TAIL, D2MI_WGRAD_MAXSPLIT: read by bare getenv before they joined the table)
    got = _tuning_in_child({"D2MI_CONV_NT": "1", "D2MI_RETINA_VAR": "0", "D2MI_CONV_TAIL": "0",
                            "D2MI_WGRAD_MAXSPLIT": "4"})
    assert got.pop("<unknown get>") == -2 ** 31 and "unknown tuning key" in got.pop("<unknown set>")
    got.pop("<retired>")
    assert got == dict(TUNING_DEFAULTS, conv_nt=1, retina_var=0, conv_tail=0, wgrad_maxsplit=4)
