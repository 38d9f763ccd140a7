"""DynamicVFE front-end on the MI355X against the CPU restatement."""
import numpy as np
import pytest
import torch

from mssvt_amd import synthetic
from oracle import vfe_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _Cfg(dict):
    def __getattr__(self, k):
        return self[k]


@pytest.mark.parametrize("pts,B,filters", [(20000, 2, [64, 128]), (160000, 1, [64, 128]), (500, 3, [16])])
def test_dynamic_vfe_matches_restatement(pts, B, filters):
    from mssvt_amd.dynamic_vfe import DynamicVFE
    p = synthetic.make_batch_points(pts, B, 3)  # rows [b, x, y, z, intensity, elongation]
    p[::97, 1] += 500.0  # some points outside the range: dropped by the reference, id -1 here
    torch.manual_seed(pts)
    vfe = DynamicVFE(_Cfg(NUM_FILTERS=filters), 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE,
                     synthetic.POINT_CLOUD_RANGE).eval()
    with torch.no_grad():
        for m in vfe.modules():  # non-trivial BatchNorm statistics
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    sd = {k: v.numpy() for k, v in vfe.state_dict().items()}
    want_f, want_c = vfe_ref.dynamic_vfe_forward(sd, p, 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE,
                                                 synthetic.POINT_CLOUD_RANGE, len(filters))
    out = vfe.to(DEV)(dict(points=torch.from_numpy(p).to(DEV), batch_size=B))
    np.testing.assert_array_equal(out["voxel_coords"].cpu().numpy(), want_c)  # integer work: bit-exact
    got = out["voxel_features"].cpu().numpy()
    assert got.shape == want_f.shape == (want_c.shape[0], filters[-1])
    # fp32 features: 1e-4 relative (fixed-point cluster centres differ from a float mean by < 1e-6 m)
    np.testing.assert_allclose(got, want_f, rtol=1e-4, atol=1e-4)
    # deterministic: the reductions are order independent
    again = vfe(dict(points=torch.from_numpy(p).to(DEV), batch_size=B))["voxel_features"]
    assert torch.equal(out["voxel_features"], again)


def test_voxel_reductions_edge_cases():
    from mssvt_amd.dynamic_vfe import voxel_max, voxel_mean_xyz
    pv = torch.tensor([2, -1, 0, 2, 2, 0], dtype=torch.int32, device=DEV)
    pts = torch.tensor([[0, 1.0, 2.0, 3.0], [0, 9, 9, 9], [0, -1, -2, -3], [0, 3, 2, 1], [0, 2, 2, 2], [0, 1, 0, -1]],
                       dtype=torch.float32, device=DEV)
    mean, cnt = voxel_mean_xyz(pts, pv, 3)
    assert cnt.tolist() == [2, 0, 3]
    np.testing.assert_allclose(mean.cpu().numpy(), [[0, -1, -2], [0, 0, 0], [2, 2, 2]], atol=1e-6)
    f = torch.tensor([[-1.0, 5.0], [100, 100], [-3, -2], [-0.5, 4], [-2, 6], [-4, -1]], device=DEV)
    mx = voxel_max(f, pv, 3).cpu().numpy()
    np.testing.assert_array_equal(mx, [[-3, -1], [-np.inf, -np.inf], [-0.5, 6]])


def test_points_to_bev_pipeline():
    """points -> DynamicVFE -> MixedScaleSparseTransformer -> dense(): the path with its two neighbours, all HIP."""
    from mssvt_amd import config
    from mssvt_amd.dynamic_vfe import DynamicVFE
    p = synthetic.make_batch_points(40000, 2, 9)
    torch.manual_seed(0)
    vfe = DynamicVFE(_Cfg(), 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE, synthetic.POINT_CLOUD_RANGE).to(DEV).eval()
    net = config.build_backbone_from_cfg().to(DEV).eval()
    with torch.no_grad():
        bd = vfe(dict(points=torch.from_numpy(p).to(DEV), batch_size=2))
        assert bd["voxel_features"].shape[1] == 128 == net.num_point_features
        sp = net(bd)["encoded_spconv_tensor"]
        bev = sp.dense()
    assert bev.shape == (2, 128, 1, 470, 470) and bool(torch.isfinite(bev).all())
    assert int((bev.abs().sum(1) > 0).sum()) == sp.features.shape[0]  # one occupied BEV cell per output voxel


@pytest.mark.parametrize("name", ["dynamic_vfe_64_128", "dynamic_vfe_16"])
def test_dynamic_vfe_matches_the_reference_run(name):
    """The HIP DynamicVFE against the reference's own DynamicVFE.forward run (oracle/gen_golden_vfe.py): same
    state-dict keys (loaded strictly), voxel coordinates bit-exact, features within 1e-4."""
    import os
    from mssvt_amd.dynamic_vfe import DynamicVFE
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    vfe = DynamicVFE(_Cfg(NUM_FILTERS=d["num_filters"].tolist()), 5, d["voxel_size"].tolist(), d["grid_size"].tolist(),
                     d["point_cloud_range"].tolist()).eval()
    sd = {k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd.")}
    vfe.load_state_dict(sd, strict=True)
    assert vfe.get_output_feature_dim() == int(d["num_point_features"])
    out = vfe.to(DEV)(dict(points=torch.from_numpy(d["points"]).to(DEV), batch_size=int(d["batch_size"])))
    np.testing.assert_array_equal(out["voxel_coords"].cpu().numpy(), d["voxel_coords"])
    got, want = out["voxel_features"].cpu().numpy(), d["voxel_features"]
    assert np.abs(got - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("pts,B", [(160000, 1), (20000, 2), (700, 3), (65, 1)])
def test_sorted_pfn_path_equals_the_atomic_path(pts, B):
    """csrc/pfn_sorted.hip (points grouped by voxel: no atomics on feature rows, x2 never stored) against round 5's atomic
    reductions (csrc/pfn_fused.hip + csrc/vfe.hip): the same arithmetic per row and order-independent reductions -- the voxel
    features must be BIT-identical, whatever the arrival order inside a voxel; voxels of 1 .. ~300 points (runs longer than a
    16-row tile and than a 64-row task window), points outside the grid, row counts that are no multiple of anything."""
    from mssvt_amd import dynamic_vfe
    p = synthetic.make_batch_points(pts, B, 11)
    p[::53, 1] += 500.0  # outside the range
    n_dense = min(300, pts // 3)
    p[5:5 + n_dense, 1:4] = p[5, 1:4] + np.random.default_rng(0).uniform(-0.02, 0.02, (n_dense, 3)).astype(np.float32)  # one crowded voxel
    p[5:5 + n_dense, 0] = p[5, 0]
    torch.manual_seed(3)
    vfe = dynamic_vfe.DynamicVFE(_Cfg(NUM_FILTERS=[64, 128]), 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE,
                                 synthetic.POINT_CLOUD_RANGE).eval()
    with torch.no_grad():
        for m in vfe.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.3)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.normal_(0, 1.0)  # negative scales too
                m.bias.normal_(0, 0.2)
    vfe = vfe.to(DEV)
    pt = torch.from_numpy(p).to(DEV)
    assert dynamic_vfe.SORTED_PFN and vfe._fused_pfn_ok(pt)
    a = vfe(dict(points=pt, batch_size=B))
    a2 = vfe(dict(points=pt, batch_size=B))
    dynamic_vfe.SORTED_PFN = False
    try:
        b = vfe(dict(points=pt, batch_size=B))
    finally:
        dynamic_vfe.SORTED_PFN = True
    assert torch.equal(a["voxel_coords"], b["voxel_coords"])
    assert torch.equal(a["voxel_features"], a2["voxel_features"])  # run to run
    assert torch.equal(a["voxel_features"], b["voxel_features"])
    assert bool(torch.isfinite(a["voxel_features"]).all()) and a["voxel_features"].shape[1] == 128
