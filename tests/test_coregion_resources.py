"""Register and scratch figures of the Coregion kernels in the built library (no GPU needed), read
the way tests/test_ard_resources.py reads the ARD ones: each new instance — the Coregion contraction
epilogue of the fused K⁻¹ = WᵀW GEMM (64- and 128-tiles), the Coregion K build and the Coregion k** —
may be no worse than the figure written in profiles/coregion.md (its table "Kernel resources"; a
spilling instance is recorded there with its scratch bytes). That the isotropic, ARD, banded, BCR and
band16 kernels were not disturbed is tests/test_kernel_resources.py's and tests/test_ard_resources.py's,
unchanged."""
import os
import re

import pytest

from tests.test_kernel_resources import _find, _kernels

COREG_MD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coregion.md")


def _recorded():
    """[(regex, vgpr, agpr, scratch)] from the rows `| `regex` | v | a | s |` of profiles/coregion.md"""
    rows = []
    for ln in open(COREG_MD, encoding="utf-8"):
        m = re.match(r"\|\s*`([^`]+)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", ln)
        if m:
            rows.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return rows


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


def test_every_coregion_instance_is_recorded():
    pats = [p for p, *_ in _recorded()]
    for want in ("gemm_kernelILi128ELb1ELb0ELi7E", "gemm_kernelILi64ELb1ELb0ELi7E", "build_coreg_kernel",
                 "predvar_coreg_kernel"):
        assert any(re.search(p, want) for p in pats), want


def test_coregion_kernels_no_worse_than_recorded(kernels):
    rows = _recorded()
    assert rows, "profiles/coregion.md has no resource table"
    for pat, v, a, scratch in rows:
        found = _find(kernels, pat)
        assert found, pat
        for name, (kv, ka, ks) in found.items():
            assert kv <= v and ka <= a and ks <= scratch, (name, (kv, ka, ks), (v, a, scratch))


def test_only_the_wtw_instances_of_the_coregion_epilogue_are_built(kernels):
    """The Coregion epilogue exists for the lower-tile WᵀW launch (opA transposed, opB not) only."""
    names = [k for k in kernels if re.search(r"gemm_kernelILi(64|128)ELb[01]ELb[01]ELi7E", k)]
    assert len(names) == 2 and all("ELb1ELb0E" in k for k in names), names
