"""GPU box: the file extraction on the ragged ICC decode.  Both pairs of entry points (porla_{kzg,ipa}_extract_batch_device,
porla_{kzg,ipa}_extract_xy_batch_device) decode every level size present in ONE ragged call per form, so the launches of a call no
longer grow with the number of sizes: files after 3, 5 and 7 writes -- all with level 0, but with level 1, level 2, and both beside
it -- issue the same launches, in calls of one file and of several.  What the calls write stays what it was: the written blocks, and
for a level recovered from its Y half the model tests/extract_xy_model.py byte for byte."""
import pytest

from tests import test_extract_gpu as te
from tests import test_extract_xy_gpu as tx
from tests.test_extract_gpu import ExFlow, check_against_written, extract

pytestmark = pytest.mark.gpu
CURVES = ["bn254", "secp256k1"]
WRITES = (3, 5, 7)                        # levels {0, 1}, {0, 2}, {0, 1, 2}


def counted(run):
    """(profile scopes recorded during run(), its result)"""
    import torch
    from porla_amd import multiexp as mx
    torch.cuda.synchronize()
    before = sum(c for _, _, c in mx.profile_get())
    res = run()
    return sum(c for _, _, c in mx.profile_get()) - before, res


@pytest.mark.parametrize("curve", CURVES)
def test_launch_count_does_not_depend_on_the_sizes_present(curve):
    import torch
    from porla_amd import multiexp as mx
    F = ExFlow(curve, torch.cuda.Stream())
    extract(F, [F.file(7)])                                       # (tables and workspaces built outside the count)
    groups = [[3, 3, 3], [5, 7, 3], [7, 7, 5]]
    mx.profile_enable(1)
    try:
        single = {t: counted(lambda: extract(F, [F.file(t)])) for t in WRITES}
        several = [counted(lambda: extract(F, [F.file(t) for t in ts])) for ts in groups]
    finally:
        mx.profile_enable(0)
    assert len({n for n, _ in single.values()}) == 1, {t: n for t, (n, _) in single.items()}
    assert [n for n, _ in several] == [single[7][0]] * len(groups), ([n for n, _ in several], single[7][0])
    for t, (_, (got,)) in single.items():
        check_against_written(F, got, t)
        assert got["counts"] == [0, 0, 0, 0] and got["row_status"] == bytes([1] * (t + te.N)), "t = %d" % t
    for ts, (_, res) in zip(groups, several):
        for t, got in zip(ts, res):
            check_against_written(F, got, t)
            assert got == single[t][1][0], "t = %d in %s" % (t, ts)


@pytest.mark.parametrize("curve", CURVES)
def test_xy_launch_count_does_not_depend_on_the_sizes_present(curve):
    """every Y half tried: the Y decodes of all sizes are one ragged call too"""
    import torch
    from porla_amd import multiexp as mx
    F = tx.XyFlow(curve, torch.cuda.Stream())
    tx.extract_xy(F, [F.file(7)], [tx.ALL])
    groups = [[3, 3, 3], [5, 7, 3]]
    mx.profile_enable(1)
    try:
        single = {t: counted(lambda: tx.extract_xy(F, [F.file(t)], [tx.ALL])) for t in WRITES}
        several = [counted(lambda: tx.extract_xy(F, [F.file(t) for t in ts], [tx.ALL] * len(ts))) for ts in groups]
    finally:
        mx.profile_enable(0)
    assert len({n for n, _ in single.values()}) == 1, {t: n for t, (n, _) in single.items()}
    assert [n for n, _ in several] == [single[7][0]] * len(groups), ([n for n, _ in several], single[7][0])
    for t, (_, (got,)) in single.items():
        check_against_written(F, got, t)
        assert got["counts"] == [0] * 6 and got["row_status_y"] == bytes([1] * t), "t = %d" % t
        assert got == tx.model_of(F, F.file(t), tx.ALL, bytes([1] * (t + te.N)), bytes([1] * t)), "t = %d" % t
    for ts, (_, res) in zip(groups, several):
        for t, got in zip(ts, res):
            assert got == single[t][1][0], "t = %d in %s" % (t, ts)


@pytest.mark.parametrize("curve", CURVES)
def test_level_2_damaged_in_x_comes_back_from_y(curve):
    import torch
    F = tx.XyFlow(curve, torch.cuda.Stream())
    f = F.file(7)
    g = tx.with_lower(f, 2, data=tx.flipped(f["lower"][2][0], 64 * (2 * te.NCOLS + 77) + 3))
    st = tx.level_statuses(7, te.N, 2, {2}, 15)
    got, = tx.extract_xy(F, [g], [tx.ALL], stream=F.stream)
    assert got["row_status"] == st and got["row_status_y"] == bytes([1] * 7)
    assert got == tx.model_of(F, g, tx.ALL, st, bytes([1] * 7))
    assert got["counts"] == [1, 0, 0, 0, 0, 0] and tx.Y_WON in got["flags"]
