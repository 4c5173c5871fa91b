"""CPU: libmmdx_hip.so loads and exports every entry point include/mmdx.h declares, and
the ctypes binding table matches the header (no compute calls: no GPU here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multi-modal-medical-imaging-and-report-ml-diagnosis-system_amd")


def _header_functions():
    src = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mmdx_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import mmdx
    if not os.path.exists(mmdx._lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8"], check=True)
    return mmdx._lib.lib()


def test_header_symbols_exported(lib):
    names = _header_functions()
    assert len(names) > 40
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mmdx.h but not exported"
    assert lib.mmdx_missing_symbols == []


def test_binding_table_matches_header():
    import mmdx
    assert sorted(mmdx._lib.SIGNATURES) == _header_functions()


def test_version_and_error_channel(lib):
    assert lib.mmdx_version() >= 1
    assert isinstance(lib.mmdx_last_error(), bytes)


def test_workspace_queries_are_host_only(lib):
    import mmdx._lib as L
    d = L.ConvDesc(128, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1, 56, 56)
    assert lib.mmdx_conv_wgrad_workspace_size(1, d) > 0
    assert lib.mmdx_gemm_workspace_size(1, 8192, 768, 768) >= 0
    assert lib.mmdx_bn_workspace_size(128 * 56 * 56, 64) > 0


def test_bn_workspace_size_skips_widths_c_is_no_multiple_of(lib):
    """mmdx_bn_workspace_size sizes for the vector widths C is a multiple of (4 channels per
    fp32 vector, 8 per bf16 one): C = 4 and C = 12 are legal fp32 BatchNorms without a bf16
    layout (C = 4 used to divide by zero on the host), C = 8 has one bf16 vector, and a C no
    kernel accepts gives 0, which every entry point's workspace check rejects."""
    import bn_ref
    assert lib.mmdx_bn_workspace_size(21, 4) == bn_ref.workspace_size(21, 4) == 4 * 8 + 5 * 4 * 4
    for rows, C in [(21, 12), (1, 8), (37, 48), (5, 2304), (128 * 56 * 56, 64), (100000, 4)]:
        want = bn_ref.workspace_size(rows, C)
        nb = max(bn_ref._rblocks(rows, C, v) for v in (4, 8) if C % v == 0)
        assert want == nb * C * 8 + 5 * C * 4 > 0
        assert lib.mmdx_bn_workspace_size(rows, C) == want, (rows, C)
        assert lib.mmdx_bn_pair_workspace_size(rows, C) == 2 * want, (rows, C)
    for C in (0, 2, 6, -8):
        assert lib.mmdx_bn_workspace_size(21, C) == 0
        assert lib.mmdx_bn_pair_workspace_size(21, C) == 0


def test_plan_op_layout_matches_c(lib):
    import ctypes
    import mmdx._lib as L
    assert lib.mmdx_plan_op_size() == ctypes.sizeof(L.PlanOp)


def _header_enum(prefix):
    src = open(os.path.join(ROOT, "include", "mmdx.h")).read()
    return {k: int(v) for k, v in re.findall(rf"\b({prefix}[A-Z0-9_]+)\s*=\s*(\d+)", src)}


def test_dtype_and_activation_codes_match_header():
    """The dtype codes the host passes (fp16 = 2 for C5) and the activation codes are the
    ones include/mmdx.h defines."""
    import mmdx._lib as L
    dt = _header_enum("MMDX_F")
    dt.update(_header_enum("MMDX_BF"))
    assert dt == {"MMDX_F32": L.F32, "MMDX_BF16": L.BF16, "MMDX_F16": L.F16}
    act = _header_enum("MMDX_ACT_")
    assert act["MMDX_ACT_NONE"] == 0 and act["MMDX_ACT_GELU"] == L.ACT_GELU
    assert act["MMDX_ACT_GELU_BWD"] == L.ACT_GELU_BWD
