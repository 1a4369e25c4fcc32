"""The instruction mix of syrk_uv16c_kernel's K loop, from the gfx950 assembly (tools/isa_mix.py; no GPU).

The kernel runs one wave per SIMD, and such a wave pays an issue turn for every instruction of its stream: an MFMA of
16 clocks hides two companions, the conversion pair or the fma pair of an operand dword, and whatever else a 32-SNP group (64 MFMAs)
holds is time.  What must be there: 16 word loads, 4 factor reads, at most 4 waits (one counted wait for the words, two for the factor
reads, the chunk boundary's), 2 scalar adds of the running word base -- 26, and 4 of slack for the loop's own branch and counters."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

GROUP = 64                              # MFMAs of a 32-SNP group
CONVERSION = ("v_cvt_scalef32_pk_f16_fp4", "v_pk_fma_f16")      # what makes an operand dword from a genotype word


@pytest.fixture(scope="module")
def report():
    import isa_mix
    from kernel_isa import make_flags
    csrc = os.path.join(ROOT, "snprelate_amd", "csrc")
    hipcc = make_flags(csrc)[0]
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    return isa_mix.report(isa_mix.assembly(csrc, "kernels_syrk_uv.hip"), "syrk_uv16c_kernel")


def test_hot_block_budget(report):
    import isa_mix
    hot = isa_mix.hottest(report)
    n_mfma = hot["count"]["mfma"]
    assert n_mfma >= 4 * GROUP and n_mfma % GROUP == 0          # the unrolled body, whole groups
    assert set(op for op in hot["ops"] if op.startswith("v_mfma")) == {"v_mfma_f32_16x16x32_f16"}
    groups = n_mfma // GROUP
    conv = sum(hot["ops"].get(op, 0) for op in CONVERSION)
    other = (hot["total"] - n_mfma - conv) / groups
    print(isa_mix.table(report))
    print("per group: %.1f instructions that are neither MFMA nor conversion, %.1f waits, %.1f scalar, %.1f vector ALU besides conversions"
          % (other, hot["count"]["waitcnt"] / groups, hot["count"]["salu"] / groups, (hot["count"]["valu"] - conv) / groups))
    assert other <= 30
    assert hot["count"]["waitcnt"] / groups <= 4
    assert hot["count"]["valu"] == conv                         # no vector address arithmetic
    assert hot["private"] == 0


def test_registers_and_no_private_access_in_any_mfma_block(report):
    assert report["info"]["VGPR"] == 256
    assert all(b["private"] == 0 for b in report["blocks"])
