"""Gray-patch features and the RVM cascade on sampled windows, the parts that need no device: the new symbols, FD_FEATURE_WHI, the
header as C99, and fd_patch_feature_length, which states the parameter rules of the three device calls."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fd_patch_feature_length", "fd_patch_extract_samples", "fd_patch_svm_evaluate_samples", "fd_patch_rvm_evaluate_samples")


def test_symbols_declared_exported_and_bound(capi):
    header = open(os.path.join(ROOT, "include", "fd_hip.h")).read()
    lib = capi.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi._SIGS and getattr(lib, name).argtypes is not None, name
    assert re.search(r"FD_FEATURE_WHI = 3\b", header) and capi.FD_FEATURE_WHI == 3
    assert (capi.FD_FEATURE_GRAY, capi.FD_FEATURE_HQ64, capi.FD_FEATURE_HISTEQ) == (0, 1, 2)   # the existing values stay
    assert re.search(r"FD_FEATURE_GRAY = 0, FD_FEATURE_HQ64 = 1, FD_FEATURE_HISTEQ = 2\b", header)
    for name in ("patch_samples_params", "patch_extract_samples", "patch_svm_evaluate_samples", "patch_rvm_evaluate_samples"):
        assert callable(getattr(capi, name)), name
    assert C.sizeof(capi.fd_patch_samples_params) == 28   # three int32, four floats, no padding


def test_header_compiles_as_c99():
    src = ('#include "fd_hip.h"\nint main(void) { fd_patch_samples_params p = {20, 20, FD_FEATURE_WHI, 1.0f, 0.0f, 1.0f, 0.390625f};\n'
           'return (int)sizeof(p) + FD_FEATURE_HISTEQ; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                   input=src.encode(), check=True)


def test_feature_length_states_the_parameter_rules(capi):
    lib = capi.lib()

    def length(pw, ph, space):
        pp = capi.patch_samples_params(pw, ph, space, 1.0 / 255.0, 0.0)
        return lib.fd_patch_feature_length(C.byref(pp))
    assert length(20, 20, capi.FD_FEATURE_GRAY) == 400
    for space in (capi.FD_FEATURE_GRAY, capi.FD_FEATURE_HQ64, capi.FD_FEATURE_HISTEQ, capi.FD_FEATURE_WHI):
        assert length(20, 20, space) == 400 and length(12, 20, space) == 240 and length(32, 32, space) == 1024
        for side in (0, 33, -1):
            assert length(side, 20, space) == -1 and length(20, side, space) == -1
    assert length(20, 20, 4) == -1 and length(20, 20, -1) == -1
    assert length(1, 1, capi.FD_FEATURE_GRAY) == 1
    assert length(1, 20, capi.FD_FEATURE_WHI) == -1     # WhiteningFilter's frequency grid divides by (side - 1)
    assert lib.fd_patch_feature_length(None) == -1


def test_null_handles_are_refused_without_a_device(capi):
    lib = capi.lib()
    bad = capi.FD_ERR_INVALID_ARGUMENT
    assert lib.fd_patch_extract_samples(None, None, None, 0, None, None, None) == bad
    assert lib.fd_patch_svm_evaluate_samples(None, None, None, None, 0, None, None, None, None) == bad
    assert lib.fd_patch_rvm_evaluate_samples(None, None, None, None, 0, None, None, None, None, None) == bad
