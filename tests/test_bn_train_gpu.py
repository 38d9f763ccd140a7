"""mssvt_bn_train_fwd / mssvt_bn_train_bwd (csrc/bn_train.hip) and ``bn_train.BnReluFunction`` against the float64 statement
of tests/bn_train_ref.py, within its derived per-element bounds: either side of the piece rule (P = 2, r - 1, r, r + 1, 2 r,
2 r + 1, 3 r + 5 with r = piece_rows(C)), at a P where a workgroup owns more than one piece and more than one workgroup runs,
on planted channels (constant, mean 1e4 / std 1, gamma = 0, gamma < 0, every element masked), with NaN / inf, with dy scaled by
powers of two, inside NaN-guarded allocations with a NaN-filled workspace, twice and on two streams, with every status code.

The ReLU mask: where the float64 pre-activation lies outside the forward bound the kernel's mask must equal the reference's;
inside it the element is undecided, the backward reference takes the kernel's own mask there, and undecided elements may make
up at most 0.1 % of a case (a condition on the inputs, see tests/test_bn_train_ref_cpu.py)."""
import functools

import numpy as np
import pytest
import torch

from mssvt_amd import _lib, bn_train
from tests import bn_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (32, 64, 128, 256)
GUARD = 64  # floats on either side of an output
MASK_CAP = 1e-3
E_BADARG, E_TOOLARGE = -1, -2


def rows_list(C):
    r = bn_train.piece_rows(C)
    assert r == ref.piece_rows(C)
    return [2, r - 1, r, r + 1, 2 * r, 2 * r + 1, 3 * r + 5]


def large_rows(C):
    """A P at which, by the launch rule, a workgroup owns two pieces and 513 workgroups run."""
    P = (ref.MAX_BLOCKS + 1) * ref.piece_rows(C) + 3
    lib = _lib.lib()
    assert lib.mssvt_bn_train_run_pieces(P, C) == 2 and lib.mssvt_bn_train_run_pieces(P - 2 * ref.piece_rows(C), C) == 1
    return P


def bhw(P):
    """(B, H, W) with B >= 2 and B H W = P."""
    B = next(b for b in range(2, P + 1) if P % b == 0)
    W = next(w for w in range(int((P // B) ** 0.5), 0, -1) if (P // B) % w == 0)
    return B, P // B // W, W


def params(k):
    return [(1e-5, 0.1), (1e-3, 0.01)][k % 2]


def reference(P, C, seed, eps, momentum):
    """Inputs, the float64 forward statement and its bounds: computed once per case and shared, read-only, among the tests (the
    one large case of each width is computed for its own test alone)."""
    return (_reference if P > 4 * ref.piece_rows(C) else _shared_reference)(P, C, seed, eps, momentum)


@functools.lru_cache(maxsize=None)
def _shared_reference(P, C, seed, eps, momentum):
    return _reference(P, C, seed, eps, momentum)


def _reference(P, C, seed, eps, momentum):
    x, dy, gamma, beta, rm, rv = ref.inputs(P, C, seed)
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    f = ref.forward_ref(x, gamma, beta, eps, momentum, rm, rv, relu=False)
    fb = ref.forward_bounds(x, gamma, beta, eps, momentum, rm, rv, ref.piece_rows(C))
    for v in (x, dy, gamma, beta, rm, rv) + tuple(f.values()) + tuple(fb.values()):
        v.setflags(write=False)
    return (x, dy, gamma, beta, rm, rv), f, fb


def guarded(n):
    """A NaN-filled allocation and the n floats in its middle."""
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())


def abi_forward(x, gamma, beta, rm, rv, eps, momentum, relu):
    """The C ABI on device tensors x (P, C), ...: every output and the workspace inside NaN guards, the workspace NaN-filled."""
    P, C = x.shape
    bufs = {k: guarded(n) for k, n in (("y", P * C), ("save_mean", C), ("save_invstd", C), ("running_mean", C), ("running_var", C),
                                       ("workspace", bn_train.workspace_bytes(P, C) // 4))}
    bufs["running_mean"][1].copy_(rm)
    bufs["running_var"][1].copy_(rv)
    _lib.call("mssvt_bn_train_fwd", x.data_ptr(), P, C, gamma.data_ptr(), beta.data_ptr(), eps, momentum,
              bufs["running_mean"][1].data_ptr(), bufs["running_var"][1].data_ptr(), int(relu), bufs["y"][1].data_ptr(),
              bufs["save_mean"][1].data_ptr(), bufs["save_invstd"][1].data_ptr(), bufs["workspace"][1].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs.values())
    out = {k: v for k, (_, v) in bufs.items() if k != "workspace"}
    out["y"] = out["y"].view(P, C)
    return out


def abi_backward(x, dy, gamma, beta, save_mean, save_invstd, relu):
    P, C = x.shape
    bufs = {k: guarded(n) for k, n in (("dx", P * C), ("dgamma", C), ("dbeta", C), ("workspace", bn_train.workspace_bytes(P, C) // 4))}
    _lib.call("mssvt_bn_train_bwd", x.data_ptr(), dy.data_ptr(), P, C, gamma.data_ptr(), beta.data_ptr(), save_mean.data_ptr(),
              save_invstd.data_ptr(), int(relu), bufs["dx"][1].data_ptr(), bufs["dgamma"][1].data_ptr(), bufs["dbeta"][1].data_ptr(),
              bufs["workspace"][1].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b, _ in bufs.values())
    out = {k: v for k, (_, v) in bufs.items() if k != "workspace"}
    out["dx"] = out["dx"].view(P, C)
    return out


def ratio(got, want, bound):
    got = got.detach().double().cpu().numpy().reshape(want.shape)
    assert np.isfinite(got).all()
    return float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())


def check_against_statement(fwd, bwd, data, f, fb, relu, P, C, what):
    """Forward outputs and gradients of one run (tensors) against the statement; returns the worst |err| / bound per output."""
    x, dy, gamma, beta, rm, rv = data
    R = ref.piece_rows(C)
    want_y = np.where(f["z"] <= 0, 0.0, f["z"]) if relu else f["z"]
    worst = dict(y=ratio(fwd["y"], want_y, fb["y"]), mean=ratio(fwd["save_mean"], f["mean"], fb["mean"]),
                 invstd=ratio(fwd["save_invstd"], f["invstd"], fb["invstd"]),
                 running_mean=ratio(fwd["running_mean"], f["running_mean"], fb["running_mean"]),
                 running_var=ratio(fwd["running_var"], f["running_var"], fb["running_var"]))
    if relu:
        got_mask = (fwd["y"] > 0).cpu().numpy().reshape(P, C)
        und = ref.undecided(f["z"], fb["z"])
        assert np.array_equal(got_mask[~und], (f["z"] > 0)[~und]), what
        assert und.mean() <= MASK_CAP, (what, und.mean())
    else:
        got_mask = np.ones((P, C), bool)
    b = ref.backward_ref(x, dy, gamma, f["mean"], f["invstd"], got_mask)
    bb = ref.backward_bounds(x, dy, gamma, f["mean"], f["invstd"], got_mask, fb, R)
    for k in ("dx", "dgamma", "dbeta"):
        worst[k] = ratio(bwd[k], b[k], bb[k])
    print("%s: worst |err| / bound %s" % (what, {k: round(v, 3) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), (what, worst)
    if relu:  # every element of this channel is masked: exact zeros
        c = ref.PLANTED["all_masked"]
        assert not bool(bwd["dx"][:, c].any()) and float(bwd["dgamma"][c]) == 0 and float(bwd["dbeta"][c]) == 0
    return worst


def on_device(data):
    return [torch.tensor(v, device=DEV) for v in data]


CASES = [(C, k) for C in WIDTHS for k in range(8)]


@pytest.mark.parametrize("C,k", CASES)
def test_c_abi_against_the_statement(C, k):
    """Values, guards, a NaN-filled workspace, two calls and two streams bit-identical; k = 7 is the large P."""
    P = rows_list(C)[k] if k < 7 else large_rows(C)
    relu = k != 3  # r + 1 runs without the ReLU
    eps, momentum = params(k)
    data, f, fb = reference(P, C, 1000 * C + k, eps, momentum)
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    x, dy, gamma, beta, rm, rv = on_device(data)
    fwd = abi_forward(x, gamma, beta, rm, rv, eps, momentum, relu)
    bwd = abi_backward(x, dy, gamma, beta, fwd["save_mean"], fwd["save_invstd"], relu)
    assert not bool(torch.isnan(fwd["y"]).any()) and not bool(torch.isnan(bwd["dx"]).any())
    check_against_statement(fwd, bwd, data, f, fb, relu, P, C, "C %d P %d relu %s" % (C, P, relu))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fwd2 = abi_forward(x, gamma, beta, rm, rv, eps, momentum, relu)
        bwd2 = abi_backward(x, dy, gamma, beta, fwd2["save_mean"], fwd2["save_invstd"], relu)
    fwd3 = abi_forward(x, gamma, beta, rm, rv, eps, momentum, relu)
    bwd3 = abi_backward(x, dy, gamma, beta, fwd3["save_mean"], fwd3["save_invstd"], relu)
    for other_f, other_b in ((fwd2, bwd2), (fwd3, bwd3)):
        assert all(torch.equal(fwd[n], other_f[n]) for n in fwd) and all(torch.equal(bwd[n], other_b[n]) for n in bwd)


def function_step(x4, dy4, gamma, beta, rm, rv, eps, momentum, relu):
    xg, w, b = x4.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = rm.clone(), rv.clone()
    y, rm_out, rv_out = bn_train.BnReluFunction.apply(xg, w, b, rm, rv, eps, momentum, relu)
    assert rm_out is rm and rv_out is rv and not rm_out.requires_grad
    y.backward(dy4)
    nhwc = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])  # noqa: E731
    return dict(y=nhwc(y.detach()), running_mean=rm, running_var=rv), dict(dx=nhwc(xg.grad), dgamma=w.grad, dbeta=b.grad), y


@pytest.mark.parametrize("C", WIDTHS)
def test_function_against_the_statement_and_the_c_abi(C):
    """Every P of the piece rule as a (B, H, W) batch with B >= 2 through the autograd Function: the bits of the C ABI."""
    for k, P in enumerate(rows_list(C)):
        relu = k != 3
        eps, momentum = params(k)
        data, f, fb = reference(P, C, 1000 * C + k, eps, momentum)
        x, dy, gamma, beta, rm, rv = on_device(data)
        B, H, W = bhw(P)
        assert B >= 2 and B * H * W == P
        x4 = x.view(B, H, W, C).permute(0, 3, 1, 2)  # channels-last in memory
        dy4 = dy.view(B, H, W, C).permute(0, 3, 1, 2)
        if k % 2:  # an NCHW input and gradient are made channels-last by the Function
            x4, dy4 = x4.contiguous(), dy4.contiguous()
        fwd, bwd, y = function_step(x4, dy4, gamma, beta, rm, rv, eps, momentum, relu)
        assert tuple(y.shape) == (B, C, H, W) and y.permute(0, 2, 3, 1).is_contiguous()
        eps32, mom32 = float(np.float32(eps)), float(np.float32(momentum))
        a_fwd = abi_forward(x, gamma, beta, rm, rv, eps32, mom32, relu)
        a_bwd = abi_backward(x, dy, gamma, beta, a_fwd["save_mean"], a_fwd["save_invstd"], relu)
        assert all(torch.equal(fwd[n], a_fwd[n]) for n in fwd) and all(torch.equal(bwd[n], a_bwd[n]) for n in bwd)
        fwd.update(save_mean=a_fwd["save_mean"], save_invstd=a_fwd["save_invstd"])
        check_against_statement(fwd, bwd, data, f, fb, relu, P, C, "Function C %d (B, H, W) = %s relu %s" % (C, (B, H, W), relu))


@pytest.mark.parametrize("C", WIDTHS)
def test_relu_false_is_plain_batch_norm(C):
    """Against torch's own batch_norm in float64 on the device, inside the statement's bounds."""
    P = 3 * ref.piece_rows(C) + 5
    eps, momentum = 1e-3, 0.01
    data, f, fb = reference(P, C, 1000 * C + 6, eps, momentum)
    x, dy, gamma, beta, rm, rv = on_device(data)
    eps32, mom32 = float(np.float32(eps)), float(np.float32(momentum))
    xd, wd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rmd, rvd = rm.double(), rv.double()
    want = torch.nn.functional.batch_norm(xd.view(1, P, C).transpose(1, 2), rmd, rvd, wd, bd, True, mom32, eps32)
    want.backward(dy.double().view(1, P, C).transpose(1, 2))
    fwd = abi_forward(x, gamma, beta, rm, rv, eps32, mom32, False)
    bwd = abi_backward(x, dy, gamma, beta, fwd["save_mean"], fwd["save_invstd"], False)
    ones = np.ones((P, C), bool)
    bb = ref.backward_bounds(data[0], data[1], data[2], f["mean"], f["invstd"], ones, fb, ref.piece_rows(C))
    for got, ref_t, bound in ((fwd["y"], want[0].t(), fb["z"]), (fwd["running_mean"], rmd, fb["running_mean"]),
                              (fwd["running_var"], rvd, fb["running_var"]), (bwd["dx"], xd.grad, bb["dx"]),
                              (bwd["dgamma"], wd.grad, bb["dgamma"]), (bwd["dbeta"], bd.grad, bb["dbeta"])):
        assert ratio(got, ref_t.detach().cpu().numpy(), bound + 1e-12 * np.abs(ref_t.detach().cpu().numpy())) <= 1.0


@pytest.mark.parametrize("C", [32, 256])
def test_scaling_dy_by_a_power_of_two_scales_the_gradients_bit_for_bit(C):
    P = 2 * ref.piece_rows(C) + 1
    data, f, fb = reference(P, C, 1000 * C + 5, *params(5))
    x, dy, gamma, beta, rm, rv = on_device(data)
    fwd = abi_forward(x, gamma, beta, rm, rv, 1e-3, 0.01, True)
    base = abi_backward(x, dy, gamma, beta, fwd["save_mean"], fwd["save_invstd"], True)
    for k in (-20, 7, 30):
        s = 2.0 ** k
        scaled = abi_backward(x, dy * s, gamma, beta, fwd["save_mean"], fwd["save_invstd"], True)
        assert all(torch.equal(scaled[n], base[n] * s) for n in base), k


@pytest.mark.parametrize("C", [32, 128])
def test_nan_and_inf_poison_only_their_own_channel(C):
    P = 3 * ref.piece_rows(C) + 5
    data, f, fb = reference(P, C, 1000 * C + 6, *params(6))
    x, dy, gamma, beta, rm, rv = on_device(data)
    eps, momentum = float(np.float32(1e-5)), float(np.float32(0.1))
    clean_f = abi_forward(x, gamma, beta, rm, rv, eps, momentum, True)
    clean_b = abi_backward(x, dy, gamma, beta, clean_f["save_mean"], clean_f["save_invstd"], True)
    bad = x.clone()
    c_nan, c_inf = 9, C - 2
    bad[P // 2, c_nan] = float("nan")
    bad[P - 1, c_inf] = float("inf")
    fwd = abi_forward(bad, gamma, beta, rm, rv, eps, momentum, True)
    bwd = abi_backward(bad, dy, gamma, beta, fwd["save_mean"], fwd["save_invstd"], True)
    keep = torch.ones(C, dtype=torch.bool, device=DEV)
    keep[c_nan] = keep[c_inf] = False
    for n in ("y", "dx"):
        got, want = (fwd if n == "y" else bwd)[n], (clean_f if n == "y" else clean_b)[n]
        assert torch.equal(got[:, keep], want[:, keep]), n
    for n in ("save_mean", "save_invstd", "running_mean", "running_var"):
        assert torch.equal(fwd[n][keep], clean_f[n][keep]), n
    for n in ("dgamma", "dbeta"):
        assert torch.equal(bwd[n][keep], clean_b[n][keep]), n
    for c in (c_nan, c_inf):  # the channel itself does not pretend to be fine
        assert not bool(torch.isfinite(fwd["save_mean"][c])) and not bool(torch.isfinite(fwd["running_mean"][c]))
        assert bool(torch.isnan(fwd["y"][:, c]).all()) and bool(torch.isnan(bwd["dgamma"][c]))
    # the same for a non-finite gradient
    bad_dy = dy.clone()
    bad_dy[1, c_nan] = float("nan")
    bad_dy[P - 2, c_inf] = float("inf")
    mask = clean_f["y"] > 0
    bad_dy[1, c_nan + 1] = float("inf")  # (masked or not: its own channel only)
    bwd = abi_backward(x, bad_dy, gamma, beta, clean_f["save_mean"], clean_f["save_invstd"], True)
    keep[c_nan + 1] = False
    assert torch.equal(bwd["dx"][:, keep], clean_b["dx"][:, keep]) and torch.equal(bwd["dgamma"][keep], clean_b["dgamma"][keep])
    assert torch.equal(bwd["dbeta"][keep], clean_b["dbeta"][keep])
    if bool(mask[1, c_nan]):
        assert bool(torch.isnan(bwd["dbeta"][c_nan]))


def test_constant_channel_gives_relu_of_beta():
    C = 64
    P = 2 * ref.piece_rows(C)
    data, f, fb = reference(P, C, 1000 * C + 4, *params(4))
    x, dy, gamma, beta, rm, rv = on_device(data)
    fwd = abi_forward(x, gamma, beta, rm, rv, 1e-5, 0.1, True)
    c = ref.PLANTED["constant"]
    assert float(fwd["save_mean"][c]) == float(x[0, c]) and float(fwd["save_invstd"][c]) == float(1 / np.sqrt(np.float32(0) + np.float32(1e-5)))
    assert bool((fwd["y"][:, c] == torch.relu(beta[c])).all())


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    assert [lib.mssvt_bn_train_supported(C) for C in (32, 64, 128, 256)] == [1, 1, 1, 1]
    assert [lib.mssvt_bn_train_supported(C) for C in (0, 16, 48, 96, 512)] == [0, 0, 0, 0, 0]
    assert [lib.mssvt_bn_train_piece_rows(C) for C in (32, 64, 128, 256, 96)] == [256, 128, 64, 32, 0]
    assert lib.mssvt_bn_train_workspace_bytes(2, 32) == ((1 + 2) * 32 + 2 * 32) * 4
    assert lib.mssvt_bn_train_workspace_bytes(513, 128) == ((9 + 2 * 9) * 128 + 2 * 128) * 4
    assert lib.mssvt_bn_train_workspace_bytes(1025 * 32 + 3, 256) == ((1026 + 2 * 513) * 256 + 2 * 256) * 4
    for P, C in ((1, 32), (0, 32), (-5, 32), (100, 96), (2 ** 31, 32), (2 ** 62, 256)):
        assert lib.mssvt_bn_train_workspace_bytes(P, C) == 0, (P, C)
        with pytest.raises(_lib.MssvtHipError):
            bn_train.workspace_bytes(P, C)
    P, C = 70, 32
    t = {k: torch.full((n,), 7.0, device=DEV) for k, n in (("x", P * C), ("dy", P * C), ("y", P * C), ("g", C), ("b", C), ("rm", C),
                                                           ("rv", C), ("m", C), ("s", C), ("dg", C), ("db", C), ("ws", 1024))}
    p = {k: v.data_ptr() for k, v in t.items()}
    fwd = lambda **kw: [kw.get(k, d) for k, d in (("x", p["x"]), ("P", P), ("C", C), ("g", p["g"]), ("b", p["b"]), ("eps", 1e-5), ("mom", 0.1),  # noqa: E731
                                                  ("rm", p["rm"]), ("rv", p["rv"]), ("relu", 1), ("y", p["y"]), ("m", p["m"]), ("s", p["s"]),
                                                  ("ws", p["ws"]), ("st", _lib.stream()))]
    bwd = lambda **kw: [kw.get(k, d) for k, d in (("x", p["x"]), ("dy", p["dy"]), ("P", P), ("C", C), ("g", p["g"]), ("b", p["b"]), ("m", p["m"]),  # noqa: E731
                                                  ("s", p["s"]), ("relu", 1), ("y", p["y"]), ("dg", p["dg"]), ("db", p["db"]), ("ws", p["ws"]),
                                                  ("st", _lib.stream()))]
    f, b = lib.mssvt_bn_train_fwd, lib.mssvt_bn_train_bwd
    for k in ("x", "g", "b", "rm", "rv", "y", "m", "s", "ws"):
        assert f(*fwd(**{k: None})) == E_BADARG, k
        assert f(*fwd(**{k: p[k] + 4})) == E_BADARG, k  # not 16-byte aligned
    for k in ("x", "dy", "g", "b", "m", "s", "y", "dg", "db", "ws"):
        assert b(*bwd(**{k: None})) == E_BADARG, k
    for bad_p in (1, 0, -3):
        assert f(*fwd(P=bad_p)) == E_BADARG and b(*bwd(P=bad_p)) == E_BADARG
    assert f(*fwd(C=0)) == E_BADARG and b(*bwd(C=-32)) == E_BADARG
    uncovered = lib.mssvt_bev_conv_wgrad(p["x"], p["dy"], 1, 7, 10, 48, 48, 3, 1, p["y"], p["ws"], _lib.stream())
    assert uncovered == E_TOOLARGE
    for bad_c in (16, 48, 512):
        assert f(*fwd(C=bad_c)) == uncovered and b(*bwd(C=bad_c)) == uncovered
    assert f(*fwd(P=2 ** 31)) == E_TOOLARGE and b(*bwd(P=2 ** 31)) == E_TOOLARGE
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in t.values())  # nothing was launched
    assert f(*fwd()) == 0 and b(*bwd()) == 0
    torch.cuda.synchronize()


def test_forward_and_backward_never_synchronise_the_host():
    C, (B, H, W) = 128, (2, 9, 11)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    dy = torch.randn(B, C, H, W, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(C).to(DEV).train()
    assert bn_train.bn_supported(bn)

    def step():
        bn.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(True)
        y = bn_train.bn_relu(bn, xg, True)
        y.backward(dy)
        return y.detach(), xg.grad

    warm = step()
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe = torch.ones(1, device=DEV)
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            out = step()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert int(bn.num_batches_tracked) == 2
    # (the running buffers moved between the two steps; the batch statistics, so y and dx, did not)
    assert torch.equal(warm[0], out[0]) and torch.equal(warm[1], out[1])
