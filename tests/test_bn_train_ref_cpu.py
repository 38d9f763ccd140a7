"""tests/bn_train_ref.py, the float64 statement the BatchNorm + ReLU kernels are held to, is itself held to torch autograd in
float64; a float32 evaluation in the kernels' order of operations stays inside every bound of the statement; and the test
inputs leave the ReLU mask undecided on far fewer elements than the cap of the GPU tests allows."""
import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import bn_train  # noqa: F401  (the module under test must import)
from tests import bn_train_ref as ref

MASK_CAP = 1e-3


def rows(t):
    """(B, C, H, W) -> (B H W, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("eps,momentum", [(1e-5, 0.1), (1e-3, 0.01)])
@pytest.mark.parametrize("relu", [True, False])
def test_statement_matches_torch_autograd_in_float64(eps, momentum, relu):
    B, C, H, W = 3, 32, 7, 5
    x, dy, gamma, beta, rm, rv = ref.inputs(B * H * W, C, 11, planted=False)
    bn = nn.BatchNorm2d(C, eps=eps, momentum=momentum).double().train()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma))
        bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(rm))
        bn.running_var.copy_(torch.from_numpy(rv))
    xt = torch.from_numpy(x).double().reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = bn(xt)
    if relu:
        out = nn.ReLU()(out)
    out.backward(torch.from_numpy(dy).double().reshape(B, H, W, C).permute(0, 3, 1, 2))
    f = ref.forward_ref(x, gamma, beta, eps, momentum, rm, rv, relu)
    mask = f["z"] > 0 if relu else np.ones(x.shape, bool)
    b = ref.backward_ref(x, dy, gamma, f["mean"], f["invstd"], mask)
    for got, want in ((f["y"], rows(out)), (f["running_mean"], bn.running_mean), (f["running_var"], bn.running_var),
                      (b["dx"], rows(xt.grad)), (b["dgamma"], bn.weight.grad), (b["dbeta"], bn.bias.grad)):
        want = want.detach().numpy()
        assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("C", [32, 64, 128, 256])
@pytest.mark.parametrize("relu", [True, False])
def test_float32_evaluation_in_kernel_order_stays_inside_the_bounds(C, relu):
    R = ref.piece_rows(C)
    worst = {}
    for P, eps, momentum in ((2, 1e-5, 0.1), (R - 1, 1e-3, 0.01), (2 * R + 1, 1e-5, 0.1), (19 * R + 5, 1e-3, 0.01)):
        eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
        x, dy, gamma, beta, rm, rv = ref.inputs(P, C, 100 + P)
        f = ref.forward_ref(x, gamma, beta, eps, momentum, rm, rv, relu)
        fb = ref.forward_bounds(x, gamma, beta, eps, momentum, rm, rv, R)
        e = ref.forward_emulated(x, gamma, beta, eps, momentum, rm, rv, relu, R)
        for k in ("y", "mean", "var", "invstd", "running_mean", "running_var"):
            ratio = np.abs(e[k].astype(np.float64) - f[k]) / np.maximum(fb[k], 1e-300)
            worst[k] = max(worst.get(k, 0.0), float(ratio.max()))
        eb = ref.backward_emulated(x, dy, gamma, beta, e["mean"], e["invstd"], relu, R)
        decided = ~ref.undecided(f["z"], fb["z"])
        if relu:
            assert np.array_equal(eb["mask"][decided], (f["z"] > 0)[decided])
            assert (~decided).mean() <= MASK_CAP
        b = ref.backward_ref(x, dy, gamma, f["mean"], f["invstd"], eb["mask"])
        bb = ref.backward_bounds(x, dy, gamma, f["mean"], f["invstd"], eb["mask"], fb, R)
        for k in ("dx", "dgamma", "dbeta"):
            ratio = np.abs(eb[k].astype(np.float64) - b[k]) / np.maximum(bb[k], 1e-300)
            worst[k] = max(worst.get(k, 0.0), float(ratio.max()))
        if relu:  # the channel whose every element is masked
            c = ref.PLANTED["all_masked"]
            assert not eb["dx"][:, c].any() and eb["dgamma"][c] == 0 and eb["dbeta"][c] == 0
    print("C %d relu %s: worst |err| / bound %s" % (C, relu, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_two_pieces_per_workgroup_in_kernel_order_stay_inside_the_bounds():
    """The P of the GPU tests' large case: more than 1024 pieces, so a workgroup merges two pieces before the merge launch."""
    C = 256
    R = ref.piece_rows(C)
    P = (ref.MAX_BLOCKS + 1) * R + 3
    assert ref.run_pieces(ref.num_pieces(P, R)) == 2
    x, dy, gamma, beta, rm, rv = ref.inputs(P, C, 1000 * C + 7)
    eps, momentum = float(np.float32(1e-3)), float(np.float32(0.01))
    f = ref.forward_ref(x, gamma, beta, eps, momentum, rm, rv, True)
    fb = ref.forward_bounds(x, gamma, beta, eps, momentum, rm, rv, R)
    e = ref.forward_emulated(x, gamma, beta, eps, momentum, rm, rv, True, R)
    eb = ref.backward_emulated(x, dy, gamma, beta, e["mean"], e["invstd"], True, R)
    und = ref.undecided(f["z"], fb["z"])
    assert und.mean() <= MASK_CAP and np.array_equal(eb["mask"][~und], (f["z"] > 0)[~und])
    b = ref.backward_ref(x, dy, gamma, f["mean"], f["invstd"], eb["mask"])
    bb = ref.backward_bounds(x, dy, gamma, f["mean"], f["invstd"], eb["mask"], fb, R)
    worst = {k: float((np.abs(e[k].astype(np.float64) - f[k]) / np.maximum(fb[k], 1e-300)).max())
             for k in ("y", "mean", "var", "invstd", "running_mean", "running_var")}
    worst.update({k: float((np.abs(eb[k].astype(np.float64) - b[k]) / np.maximum(bb[k], 1e-300)).max()) for k in ("dx", "dgamma", "dbeta")})
    print("worst |err| / bound %s" % {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_mask_cap_holds_for_the_test_inputs():
    """On the Gaussian inputs the GPU tests use, the elements whose pre-activation lies inside the forward bound -- where the
    float32 mask may differ from the float64 one -- are far fewer than the cap, and no element outside that band flips."""
    for C in (32, 256):
        R = ref.piece_rows(C)
        P = 40 * R + 3
        x, dy, gamma, beta, rm, rv = ref.inputs(P, C, 5)
        eps, momentum = float(np.float32(1e-3)), float(np.float32(0.01))
        f = ref.forward_ref(x, gamma, beta, eps, momentum, rm, rv, True)
        fb = ref.forward_bounds(x, gamma, beta, eps, momentum, rm, rv, R)
        e = ref.forward_emulated(x, gamma, beta, eps, momentum, rm, rv, True, R)
        und = ref.undecided(f["z"], fb["z"])
        print("C %d: %.2e of %d elements undecided" % (C, und.mean(), und.size))
        assert und.mean() <= MASK_CAP / 10
        assert np.array_equal((e["z"] > 0)[~und], (f["z"] > 0)[~und])


def test_bounds_are_tight_enough_to_tell_a_wrong_kernel():
    """The plain E[x^2] - E[x]^2 in float32 leaves the bound by orders of magnitude on the mean 1e4 / std 1 channel."""
    C, R = 32, ref.piece_rows(32)
    P = 3 * R + 5
    x, dy, gamma, beta, rm, rv = ref.inputs(P, C, 9)
    f = ref.forward_ref(x, gamma, beta, 1e-5, 0.1, rm, rv)
    fb = ref.forward_bounds(x, gamma, beta, 1e-5, 0.1, rm, rv, R)
    c = ref.PLANTED["far_mean"]
    s = np.float32(0)
    s2 = np.float32(0)
    for v in x[:, c]:
        s += v
        s2 += v * v
    naive = float(s2 / np.float32(P) - (s / np.float32(P)) ** 2)
    assert abs(naive - f["var"][c]) > 100 * fb["var"][c]
