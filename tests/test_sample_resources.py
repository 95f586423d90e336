"""Register and scratch figures of the sampler's kernels in the built library (no GPU needed), read
the way tests/test_coregion_resources.py reads the Coregion ones: every kernel of gpx_sample.hip is
listed in profiles/samples.md (its table "Kernel resources") and none is worse than its recorded
VGPR / AGPR / scratch figures — the step kernel keeps a panel row of 64 doubles in registers, and a
spill there turns every block step's substitution into scratch traffic. The trailing update and the
product are instances of the library's GEMM that existed before (gemm_kernel<.., EPI_STORE>)."""
import os
import re

import pytest

from tests.test_kernel_resources import _find, _kernels

SAMPLES_MD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "samples.md")


def _recorded():
    """[(regex, vgpr, agpr, scratch)] from the rows `| `regex` | v | a | s |` of profiles/samples.md"""
    rows = []
    for ln in open(SAMPLES_MD, encoding="utf-8"):
        m = re.match(r"\|\s*`([^`]+)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", ln)
        if m:
            rows.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return rows


@pytest.fixture(scope="module")
def kernels():
    return _kernels()


def test_every_sampler_kernel_is_recorded(kernels):
    pats = [p for p, *_ in _recorded()]
    built = [k for k in kernels if re.search(r"gpx\d+sample_\w+_kernel", k)]
    assert len(built) == 4, built   # iota, load, step, out
    for name in built:
        assert any(re.search(p, name) for p in pats), name


def test_sampler_kernels_no_worse_than_recorded(kernels):
    rows = _recorded()
    assert rows, "profiles/samples.md has no resource table"
    for pat, v, a, scratch in rows:
        for name, (kv, ka, ks) in _find(kernels, pat).items():
            assert kv <= v and ka <= a and ks <= scratch, (name, (kv, ka, ks), (v, a, scratch))


def test_the_step_kernel_does_not_spill(kernels):
    for name, (v, a, scratch) in _find(kernels, r"sample_step_kernel").items():
        assert scratch == 0 and v + a <= 256, (name, v, a, scratch)   # (two workgroups' waves per SIMD)
