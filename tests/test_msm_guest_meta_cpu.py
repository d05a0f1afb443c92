"""Kernel descriptors of the MSM's guest kernels in the built library (tools/kernel_meta.py: metadata of the gfx950 code objects, no
device needed): what runs beside a guest-room accumulation must fit the room it leaves."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "porla_amd", "libmultiexp.so")

# every kernel of the pipelined tree plan, and the combine in front of them
GUESTS = ["k_tree_level<porla::Bn254G1>", "k_tree_level_quad<porla::Bn254G1>", "k_tree_tail<porla::Bn254G1, true>",
          "k_bucket_combine<porla::Bn254G1>"]


@pytest.fixture(scope="module")
def meta():
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "tools", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    import subprocess
    rows = [k for blob in km.code_objects(LIB) for k in km.kernels(blob)]
    names = subprocess.run([km.CXXFILT], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    assert len(names) == len(rows) and rows
    out = {}
    for r, nm in zip(rows, names):
        out.setdefault(nm.replace("void ", "").split("(")[0], []).append(r)
    return out


def test_guest_room_accumulation_leaves_the_room_it_promises(meta):
    """three blocks per compute unit by the LDS request alone (no static LDS; more than a quarter, at most a third of 160 KB), and
    three waves per SIMD of its allocation (granule 8) leave at least the 128 registers a guest takes"""
    import re
    src = open(os.path.join(ROOT, "porla_amd", "csrc", "msm.hip.h")).read()
    m = re.search(r"BUCKET_SUM_GUEST_LDS = (\d+) \* 1024;", src)
    assert m
    lds = int(m.group(1)) * 1024
    assert 160 * 1024 // 4 < lds <= 160 * 1024 // 3
    recs = meta.get("porla::k_bucket_sum30<porla::Bn254G1>")
    assert recs
    for r in recs:
        assert int(r["group_segment_fixed_size"]) == 0, r
        alloc = (int(r["vgpr_count"]) + 7) // 8 * 8
        assert 512 - 3 * alloc >= 128, r
        assert int(r["vgpr_spill_count"]) == 0, r


@pytest.mark.parametrize("kernel", GUESTS)
def test_guest_kernels_fit_128_registers_without_vector_spills(meta, kernel):
    recs = meta.get("porla::" + kernel)
    assert recs, "no descriptor for %s" % kernel
    for r in recs:
        assert int(r["vgpr_count"]) <= 128, r
        assert int(r["vgpr_spill_count"]) == 0, r
