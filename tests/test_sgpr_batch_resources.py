"""Register, scratch and LDS figures of the fused small-shape SGPR kernels in the built library (no
GPU needed), read the way tests/test_svgp_batch_resources.py reads the SVGP ones: every instance of
sgpr_small_kernel<DM, NT> and sgpr_small_predict_kernel<DM> may be no worse than the figure written
in profiles/sgpr_batch.md (its table "Kernel resources"; an instance that spills is recorded there
with its scratch bytes, and the profile says where they come from). That the other kernels were not
disturbed is tests/test_kernel_resources.py's and tests/test_svgp_batch_resources.py's, unchanged."""
import os
import re
import subprocess
import tempfile

import pytest

from portfoliooptgp_amd import _native as N
from tests.test_kernel_resources import BUNDLER, MAGIC, OBJCOPY, READELF

MD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sgpr_batch.md")
LDS_LIMIT = 160 * 1024  # bytes of LDS a gfx950 workgroup may use


def _recorded():
    """[(regex, vgpr, agpr, scratch, lds)] from the rows `| `regex` | v | a | s | lds |` of the profile"""
    rows = []
    for ln in open(MD, encoding="utf-8"):
        m = re.match(r"\|\s*`([^`]+)`\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|\s*(\d+)\s*\|", ln)
        if m:
            rows.append((m.group(1),) + tuple(int(m.group(i)) for i in range(2, 6)))
    return rows


def _small_kernels():
    """{kernel symbol: (vgpr_count, agpr_count, private_segment_fixed_size, group_segment_fixed_size)} of the
    sgpr_small kernels in libgpx.so's gfx950 code objects."""
    if not (os.path.exists(N.LIB_PATH) and all(os.path.exists(t) for t in (BUNDLER, OBJCOPY, READELF))):
        pytest.skip("libgpx.so or the ROCm LLVM tools are absent")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fatbin")
        subprocess.run([OBJCOPY, "--dump-section", f".hip_fatbin={fb}", N.LIB_PATH], check=True)
        data = open(fb, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
        for i, s in enumerate(starts):
            chunk = os.path.join(d, f"b{i}")
            with open(chunk, "wb") as f:
                f.write(data[s:starts[i + 1] if i + 1 < len(starts) else len(data)])
            co = os.path.join(d, f"b{i}.co")
            r = subprocess.run([BUNDLER, "--unbundle", "--type=o", f"--input={chunk}",
                                "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
            if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
                continue
            notes = subprocess.run([READELF, "--notes", co], capture_output=True, text=True).stdout
            for block in re.split(r"\n\s+- \.", notes):
                m = re.search(r"\.?name:\s+(\S+)", block)
                if not m or "sgpr_small" not in m.group(1):
                    continue

                def g(k):
                    f = re.search(k + r":\s+(\d+)", block)
                    return int(f.group(1)) if f else 0
                out[m.group(1)] = (g(r"\.vgpr_count"), g(r"agpr_count"), g(r"\.private_segment_fixed_size"),
                                   g(r"\.group_segment_fixed_size"))
    return out


@pytest.fixture(scope="module")
def kernels():
    return _small_kernels()


def test_every_instance_is_built_and_recorded(kernels):
    pats = [p for p, *_ in _recorded()]
    want = [f"sgpr_small_kernelILi{dm}ELi{nt}E" for dm in (1, 2, 4, 8, 16) for nt in (1, 4)]
    want += [f"sgpr_small_predict_kernelILi{dm}E" for dm in (1, 2, 4, 8, 16)]
    for w in want:
        assert any(w in k for k in kernels), w
        assert sum(1 for p in pats if re.search(p, w)) == 1, w
    assert len(kernels) == len(want), sorted(kernels)
    assert not [k for k in kernels if "svgp_small" in k]  # the SVGP table's count stays its own


def test_kernels_no_worse_than_recorded(kernels):
    rows = _recorded()
    assert rows, "profiles/sgpr_batch.md has no resource table"
    for pat, v, a, scratch, lds in rows:
        hits = {k: f for k, f in kernels.items() if re.search(pat, k)}
        assert hits, pat
        for name, (kv, ka, ks, kl) in hits.items():
            print(name, (kv, ka, ks, kl), "recorded", (v, a, scratch, lds))
            assert kv <= v and ka <= a and ks <= scratch and kl <= lds, (name, (kv, ka, ks, kl), (v, a, scratch, lds))


def test_lds_within_a_workgroup(kernels):
    """Every instance fits a workgroup's 160 KiB of LDS."""
    for name, (_, _, _, lds) in kernels.items():
        assert lds <= LDS_LIMIT, (name, lds)
