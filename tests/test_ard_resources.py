"""Register and scratch figures of the ARD kernels in the built library (no GPU needed), read the
way tests/test_kernel_resources.py reads them: each new instance — the ARD contraction epilogues of
the fused K⁻¹ = WᵀW GEMM (64- and 128-tiles, the two-term and the GPX_MAX_TERMS instance), the ARD
K build and the ARD k** — may be no worse than the figure written in profiles/ard.md (its table
"Kernel resources"; a spilling instance is recorded there with its scratch bytes). That the banded,
BCR and band16 kernels were not disturbed is tests/test_kernel_resources.py's, unchanged."""
import os
import re

import pytest

from tests.test_kernel_resources import _find, _kernels

ARD_MD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "ard.md")


def _recorded():
    """[(regex, vgpr, agpr, scratch)] from the rows `| `regex` | v | a | s |` of profiles/ard.md"""
    rows = []
    for ln in open(ARD_MD, encoding="utf-8"):
        m = re.match(r"\|\s*`([^`]+)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", ln)
        if m:
            rows.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return rows


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


def test_every_ard_instance_is_recorded():
    pats = [p for p, *_ in _recorded()]
    for want in ("gemm_kernelILi128ELb1ELb0ELi5E", "gemm_kernelILi128ELb1ELb0ELi6E", "gemm_kernelILi64ELb1ELb0ELi5E",
                 "gemm_kernelILi64ELb1ELb0ELi6E", "build_ard_kernel", "predvar_ard_kernel"):
        assert any(re.search(p, want) for p in pats), want


def test_ard_kernels_no_worse_than_recorded(kernels):
    rows = _recorded()
    assert rows, "profiles/ard.md has no resource table"
    for pat, v, a, scratch in rows:
        for name, (kv, ka, ks) in _find(kernels, pat).items():
            print(name, (kv, ka, ks), "recorded", (v, a, scratch))
            assert kv <= v and ka <= a and ks <= scratch, (name, (kv, ka, ks), (v, a, scratch))


def test_only_the_wtw_instances_of_the_ard_epilogue_are_built(kernels):
    """The ARD epilogue exists for the lower-tile WᵀW launch (opA transposed, opB not) only."""
    names = [k for k in kernels if re.search(r"gemm_kernelILi(64|128)ELb[01]ELb[01]ELi[56]E", k)]
    assert len(names) == 4 and all("ELb1ELb0E" in k for k in names), names
