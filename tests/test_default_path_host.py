"""No GPU: the kernels of the default path (prep, guidance, reduction) are templates over the record source (psm_kernels.h, Recs), and
the built library holds both instantiations of each - the pair by value in the kernarg, RecVal<PcPair, 1>, and the batch's device
table, const PcPair * - and no entry with the loose per-pair pointers they took before."""
import re
import subprocess

import pytest

BY_VALUE, TABLE = "NS_6RecValINS_6PcPairELi1EEE", "PKNS_6PcPairE"
# kernel, its template arguments ahead of the source
KERNELS = (("k_prep", "Lb0E"), ("k_prep", "Lb1E"), ("k_prep_u8", ""), ("k_guide_march", "Li0E"), ("k_guide_march", "Li1E"),
           ("k_guide_march", "Li2E"), ("k_chunk_min", ""))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as G
    G.build()
    from primestereomatch_amd import capi
    return capi


def test_library_holds_both_instantiations_and_no_other(built):
    out = subprocess.run(["nm", "-D", "--defined-only", built.LIB_PATH], capture_output=True, text=True, check=True).stdout
    blob = open(built.LIB_PATH, "rb").read()
    kept = set()
    for kernel, head in KERNELS:
        stem = rf"_ZN3psm{len(kernel)}{kernel}I{head}"
        by_value = re.search(rf"\bV ({stem}{BY_VALUE}EEv\w+)$", out, re.M)
        table = re.search(rf"\bV ({stem}{TABLE}EEv\w+)$", out, re.M)
        assert by_value and table, (kernel, head)
        assert by_value.group(1) != table.group(1)
        for sym in (by_value.group(1), table.group(1)):
            assert (sym + ".kd").encode() in blob, sym
            kept.add(sym)
    # every device symbol of these names is one of the fourteen above: nothing is left of the signatures with loose pointers
    names = {kernel for kernel, _ in KERNELS}
    theirs = {m.group(1) for m in re.finditer(r"\b[VDBW] (_ZN3psm\d+(k_\w+?)(?:I\w+|E\w+))$", out, re.M) if m.group(2) in names}
    assert theirs == kept, sorted(theirs ^ kept)
    assert len(kept) == 2 * len(KERNELS)
