"""The float64 statement of the VFE run operators (tests/vfe_train_ref.py) against torch autograd in float64 on the CPU, on
the case set the GPU tests use: ``scatter_reduce("amax", include_self=False)``, ``index_add`` and ``[inv]`` -- the
expressions of ``DynamicVFE._forward_train``.  This validates the yardstick; it does not touch the HIP kernels.

One difference from the torch branch is deliberate.  ``_forward_train`` reduces into a ZERO tensor, and torch's backward of
``scatter_reduce("amax", include_self=False)`` counts that seed as one more tie wherever a run's maximum is exactly 0 (it
divides by count + 1 there).  The statement divides by the number of ROWS that attain the maximum, everywhere; the autograd
expression here therefore reduces into -inf (no seed can tie) and zeroes the empty runs afterwards.  In the VFE the reduced
values are ReLU outputs, whose backward is zero exactly where the maximum is 0, so no parameter gradient sees the difference
(tests/test_vfe_train_fused_gpu.py compares them with the torch branch)."""
import numpy as np
import pytest
import torch

from tests import vfe_train_ref as ref


def _inv(run_off):
    return torch.from_numpy(np.repeat(np.arange(len(run_off) - 1), np.diff(run_off)))


def _per_voxel_max(v, inv, N):
    idx = inv.unsqueeze(1).expand_as(v)
    out = torch.full((N, v.shape[1]), -np.inf, dtype=v.dtype).scatter_reduce(0, idx, v, "amax", include_self=False)
    return torch.where(torch.isinf(out) & (out < 0), torch.zeros_like(out), out)


@pytest.mark.parametrize("table,F", ref.CASES)
def test_run_operators_match_autograd(table, F):
    c = ref.make_case(table, F)
    inv, N = _inv(c["run_off"]), len(c["run_off"]) - 1
    x = torch.from_numpy(c["x"].astype(np.float64)).requires_grad_()
    cat = torch.cat((x, _per_voxel_max(x, inv, N)[inv]), dim=-1)
    assert np.array_equal(cat.detach().numpy(), c["cat"])
    (gx,) = torch.autograd.grad((cat * torch.from_numpy(c["g_cat"].astype(np.float64))).sum(), x)
    np.testing.assert_allclose(gx.numpy(), c["gx_cat"], rtol=1e-12, atol=1e-12 * float(np.abs(c["g_cat"]).max()))
    mx = _per_voxel_max(x, inv, N)
    assert np.array_equal(mx.detach().numpy(), c["max"])
    (gx,) = torch.autograd.grad((mx * torch.from_numpy(c["g_max"].astype(np.float64))).sum(), x)
    np.testing.assert_allclose(gx.numpy(), c["gx_max"], rtol=1e-12, atol=0)
    assert (c["bound_cat"] >= 0).all() and (c["bound_max"] >= 0).all()


def test_the_planted_rows_are_there():
    c = ref.make_case("mixed", 64)
    kinds = {k for k, _ in c["planted"]}
    assert kinds == {"tie2", "tie3", "negative", "zeros", "huge"}, kinds
    x, off = c["x"], c["run_off"]
    for kind, v in c["planted"]:
        s, e = off[v], off[v + 1]
        hits = (x[s:e] == x[s:e].max(axis=0)).sum(axis=0)
        if kind == "tie2":
            assert (hits == 2).all() and (c["gx_cat"][s] - c["g_cat"][s, :64] != 0).all()
        if kind == "tie3":
            assert (hits == 3).all()
        if kind == "negative":
            assert (c["max"][v] < 0).all()
        if kind == "zeros":
            assert hits[0] == e - s and hits[63] == e - s and c["max"][v, 0] == 0
    lengths = set(c["lengths"])
    assert {0, 1, 2, 3, 15, 16, 17, 63, 64, 65, ref.CHUNK - 1, ref.CHUNK, ref.CHUNK + 1, 3 * ref.CHUNK + 5, 1000} <= lengths


@pytest.mark.parametrize("name", sorted(ref.grouping_cases()))
def test_grouping_matches_unique(name):
    pv, N = ref.grouping_cases()[name]
    order, run_off = ref.group(pv, N)
    kept = pv[order]
    assert (kept >= 0).all() and (np.diff(kept) >= 0).all() and len(order) == int((pv >= 0).sum()) == run_off[-1]
    for v in range(min(N, 50)):
        rows = order[run_off[v]:run_off[v + 1]]
        assert (pv[rows] == v).all() and (np.diff(rows) > 0).all()
    # torch.unique's inverse on the kept points is the voxel of every point when every id is carried; here ids may be missing
    _, counts = np.unique(kept, return_counts=True)
    assert sorted(np.diff(run_off)[np.diff(run_off) > 0].tolist()) == sorted(counts.tolist())


@pytest.mark.parametrize("cluster,centre,distance,npf", [(True, True, False, 5), (True, True, True, 4), (False, True, False, 5),
                                                         (True, False, True, 3)])
def test_augmentation_matches_the_torch_branch_expressions(cluster, centre, distance, npf):
    rng = np.random.default_rng(3)
    P, N = 500, 37
    pts = np.concatenate((rng.integers(0, 2, (P, 1)), rng.uniform(-3, 3, (P, 5))), axis=1).astype(np.float32)
    pv = rng.integers(-1, N, P).astype(np.int32)
    coords = rng.integers(0, 30, (N, 4)).astype(np.int32)
    vs, off = [0.3, 0.2, 0.5], [-2.85, -2.9, -0.75]
    order, run_off = ref.group(pv, N)
    got = ref.augment(pts, order, run_off, coords, vs, off, npf, cluster, centre, distance)
    p = torch.from_numpy(pts.astype(np.float64))[torch.from_numpy(order.astype(np.int64))]
    inv = _inv(run_off)
    xyz = p[:, 1:4]
    cols = [p[:, 1:npf + 1]]
    if cluster:
        tot = torch.zeros((N, 3), dtype=p.dtype).index_add(0, inv, xyz)
        cnt = torch.zeros(N, dtype=p.dtype).index_add(0, inv, torch.ones_like(inv, dtype=p.dtype))
        cols.append(xyz - (tot / cnt.clamp(min=1).unsqueeze(1))[inv])
    if centre:
        cell = torch.from_numpy(coords[:, [3, 2, 1]].astype(np.float64))[inv]
        cols.append(xyz - (cell * torch.tensor(vs, dtype=torch.float32).double() + torch.tensor(off, dtype=torch.float32).double()))
    if distance:
        cols.append(torch.norm(xyz, p=2, dim=1, keepdim=True))
    np.testing.assert_allclose(got, torch.cat(cols, dim=-1).numpy(), rtol=1e-13, atol=1e-13)
