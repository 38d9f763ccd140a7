"""The four matrix kernels every gradient of the backbone flows through, at their tile edges, through the C ABI, against
the float64 statements and per-element bounds of tests/train_matrix_ref.py (held to torch by
tests/test_train_matrix_ref_cpu.py):

a. mssvt_linear_wgrad (csrc/linear_wgrad.hip): the 7 tiled forms, the 7 k_wgrad_partial<TPW> forms, k_wgrad_reduce with
   one, two, nine slices and the slice counts either side of one slice per CU and of two per CU;
b. mssvt_linear_rows (4 shapes) and mssvt_linear_rows_h (6 shapes): every epilogue form, strided X and Y, the second
   round of the persistent loop, and for the split-fp16 kernel rows outside the range of the normalisation;
c. mssvt_pair_attention_fwd / _bwd (csrc/pair_attn.hip): the 30 instantiations on a hand-built window list.

Two comparisons.  EXACT: small-integer operands (times a power of two per row for the linear kernels), every partial
sum an integer below 2^24, so the result is the same in any order and the kernel must return its bits: a dropped,
doubled or misplaced row fails at any M.  BOUNDED: random operands with rows at scales 2^-8 .. 2^8, every element
inside the bound derived for it.  Outputs are NaN-prefilled inside sentinel-filled allocations; inputs lie between 1e30.

Worst |err| / bound over this file, measured on the MI355X (`pytest -s` prints every one):
    mssvt_linear_wgrad        dW 0.53, db 0.39
    mssvt_linear_rows         0.25
    mssvt_linear_rows_h       0.061 (the 2^126 row 0.024, the [2^127, FLT_MAX] row 0.021, the subnormal row 0.000)
    mssvt_pair_attention_fwd  O 0.047, lse 0.15
    mssvt_pair_attention_bwd  dq 0.31, dkv 0.45"""
import functools
import types

import pytest
import torch

from mssvt_amd import _lib
from tests import train_matrix_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, BADARG, TOOLARGE = 0, -1, -2
NAN = float("nan")  # prefill of every output: an element the kernel does not write fails every comparison
SENT = -777.25  # prefill of the columns / rows a kernel must leave alone
G = 256  # guard floats around every output


def _inside(got, want, lim, what):
    """|got - want| <= lim elementwise; prints the worst ratio first (the figure to read when it fails)."""
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("%s: worst |err| / bound = %.3f" % (what, ratio))
    assert bool((err <= lim).all()), (what, ratio)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _junk():
    """An unrelated allocation between two runs: the second run's buffers land elsewhere."""
    return torch.empty(1 << 18, device=DEV).normal_()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _on_second_stream(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fn()
    s.synchronize()
    return out


def _scaled_rows(M, K, g):
    return torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float())


# ---------------------------------------------------------------------------------------------------------
# a. mssvt_linear_wgrad
# ---------------------------------------------------------------------------------------------------------

# (Cout, Cin) = (64 OW, 16 NTC) of WG_TILED: (4, 8) (2, 16) (2, 8) (2, 4) (1, 4) (1, 8) (4, 4)
WG_TILED = [(256, 128), (128, 256), (128, 128), (128, 64), (64, 64), (64, 128), (256, 64)]
# k_wgrad_partial<TPW>: tiles = ceil(Cout / 16) (ceil(Cin / 16) + bias), tpw = ceil(tiles / 4 waves), TPW = the next of 1 2 4 8 16 32 40
#   (Cout, Cin)   nto ntc   tiles +b / -b   tpw +b / -b   TPW
#   (16, 16)        1   1        2 / 1          1 / 1       1
#   (20, 36)        2   3        8 / 6          2 / 2       2     (neither a multiple of 16: the zero-padded tile columns)
#   (48, 64)        3   4       15 / 12         4 / 3       4
#   (80, 80)        5   5       30 / 25         8 / 7       8
#   (96, 144)       6   9       60 / 54        15 / 14     16
#   (192, 144)     12   9      120 / 108       30 / 27     32
#   (256, 144)     16   9      160 / 144       40 / 36     40     (160 tiles: the limit)
WG_PARTIAL = [(16, 16), (20, 36), (48, 64), (80, 80), (96, 144), (192, 144), (256, 144)]
# rows: one slice (rows_per_slice = 64 at these sizes) with 1 .. 4 staging steps whose last is partial, full or one over;
# two slices (65 .. 81); nine slices (513, 576): the reduce's eight groups wrap
WG_ROWS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 79, 80, 81, 64 * 8 + 1, 64 * 9)


def _wg_tpw(cout, cin, bias):
    return -(-((cout + 15) // 16 * ((cin + 15) // 16 + (1 if bias else 0))) // 4)


def test_wgrad_shapes_reach_every_instantiation():
    """The tile arithmetic of the table above, and none of the partial shapes is a tiled one."""
    assert not set(WG_PARTIAL) & set(WG_TILED)
    for (cout, cin), lo, hi in zip(WG_PARTIAL, (1, 2, 3, 5, 9, 17, 33), (1, 2, 4, 8, 16, 32, 40)):
        for bias in (True, False):
            assert lo <= _wg_tpw(cout, cin, bias) <= hi, (cout, cin, bias)
    assert 16 * (9 + 1) == 160


def _wg_run(M, cin, cout, x, dy, with_db, stream=None):
    """One call inside guarded allocations.  Returns (dW, db or None) on the GPU after checking every word outside them."""
    assert M == 0 or (x.shape == (M, cin) and dy.shape == (M, cout))  # the kernel reads M rows of each
    need = int(_lib.lib().mssvt_linear_wgrad_workspace_floats(M, cin, cout))
    ws = torch.full((need + G,), NAN, device=DEV)  # exactly `need` floats are the kernel's; the tail must stay NaN
    buf = torch.full((3 * G + cout * cin + cout,), SENT, device=DEV)
    dw, db = buf[G:G + cout * cin], buf[2 * G + cout * cin:2 * G + cout * cin + cout]
    dw.fill_(NAN)
    if with_db:
        db.fill_(NAN)
    _lib.call("mssvt_linear_wgrad", M, cin, cout, _lib.ptr(x), _lib.ptr(dy), dw.data_ptr(), db.data_ptr() if with_db else None,
              _lib.ptr(ws), _lib.stream() if stream is None else stream)
    out = buf.clone()
    keep = torch.ones_like(out, dtype=torch.bool)
    keep[G:G + cout * cin] = False
    if with_db:
        keep[2 * G + cout * cin:2 * G + cout * cin + cout] = False
    assert bool((out[keep] == SENT).all()), "a word outside dW / db changed"
    assert bool(torch.isnan(ws[need:]).all()), "the workspace was written past its size"
    return dw.view(cout, cin).clone(), (db.clone() if with_db else None)


@functools.lru_cache(maxsize=None)
def _wg_case(cout, cin):
    g = torch.Generator().manual_seed(1000 * cout + cin)
    M = max(WG_ROWS)
    c = types.SimpleNamespace()
    c.xi = torch.randint(-3, 4, (M, cin), generator=g).float()
    c.dyi = torch.randint(-3, 4, (M, cout), generator=g).float()
    c.hot = torch.zeros(M, cout)
    c.hot[torch.arange(M), torch.arange(M) % cout] = 1.0  # dW[o] = the sum of the X rows m = o (mod Cout), db[o] their count
    c.xr, c.dyr = _scaled_rows(M, cin, g), _scaled_rows(M, cout, g)
    c.d = types.SimpleNamespace(**{k: getattr(c, k).to(DEV) for k in ("xi", "dyi", "hot", "xr", "dyr")})
    return c


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("cout,cin", WG_TILED + WG_PARTIAL)
def test_wgrad_every_form_at_the_slice_edges(cout, cin, with_db):
    c = _wg_case(cout, cin)
    for M in WG_ROWS:
        for x, dy, xd, dyd in ((c.xi, c.dyi, c.d.xi, c.d.dyi), (c.xi, c.hot, c.d.xi, c.d.hot)):
            dw, db, mw, mb = ref.wgrad_ref(x[:M], dy[:M])
            assert float(mw.max()) < 2 ** 24 and float(mb.max()) < 2 ** 24
            gw, gb = _wg_run(M, cin, cout, xd[:M].contiguous(), dyd[:M].contiguous(), with_db)
            assert torch.equal(gw.cpu().double(), dw), ("exact dW", M)
            assert gb is None or torch.equal(gb.cpu().double(), db), ("exact db", M)
        dw, db, mw, mb = ref.wgrad_ref(c.xr[:M], c.dyr[:M])
        gw, gb = _wg_run(M, cin, cout, c.d.xr[:M].contiguous(), c.d.dyr[:M].contiguous(), with_db)
        _inside(gw, dw, ref.wgrad_bound(M, mw), "mssvt_linear_wgrad dW (%d, %d) M = %d" % (cout, cin, M))
        if with_db:
            _inside(gb, db, ref.wgrad_bound(M, mb), "mssvt_linear_wgrad db (%d, %d) M = %d" % (cout, cin, M))


@pytest.mark.parametrize("cout,cin", [(16, 16), (64, 64)])
def test_wgrad_exact_at_the_grid_edges(cout, cin):
    """M = 64 cus - 1, 64 cus, 64 cus + 1: one slice per CU with the last slice short, full, and one row over
    (rows_per_slice 64 -> 80); M = 2048 cus - 1, 2048 cus: the switch to two slices per CU.  Exact operands (a rounding
    bound says nothing at half a million rows); every other row of dY a one-hot, so a lost row is an identifiable one."""
    cus = _cus()
    Mx = 2048 * cus
    assert 3 * 3 * Mx < 2 ** 24
    g = torch.Generator().manual_seed(cout)
    x = torch.randint(-3, 4, (Mx, cin), generator=g, dtype=torch.float32)
    dy = torch.randint(-3, 4, (Mx, cout), generator=g, dtype=torch.float32)
    odd = torch.arange(1, Mx, 2)
    dy[odd] = 0.0
    dy[odd, (odd // 2) % cout] = 1.0
    xd, dyd = x.to(DEV), dy.to(DEV)
    # float64 sums over the first a rows, then row by row (an outer product each) up to the next sizes
    for a, more in ((64 * cus - 1, 2), (Mx - 1, 1)):
        dw, db = dy[:a].double().t() @ x[:a].double(), dy[:a].double().sum(0)
        for M in range(a, a + more + 1):
            if M > a:
                dw, db = dw + torch.outer(dy[M - 1].double(), x[M - 1].double()), db + dy[M - 1].double()
            gw, gb = _wg_run(M, cin, cout, xd[:M], dyd[:M], True)
            assert torch.equal(gw.cpu().double(), dw) and torch.equal(gb.cpu().double(), db), M


def test_wgrad_zero_rows_and_refusals():
    """M = 0 zeroes both outputs.  BADARG: Cin % 4, Cout % 4, a NULL pointer.  TOOLARGE: more than 160 tiles -- with the
    bias column (256, 160) is 176 tiles and refused, without it 160 and served; (112, 352) is 7 x 23 = 161 with it.
    Refusals leave dW and db untouched; train_path.wgrad_supported agrees with the with-bias answer."""
    from mssvt_amd import train_path
    lib, st, p = _lib.lib(), _lib.stream(), _lib.ptr
    x, dy = torch.ones(4, 16, device=DEV), torch.ones(4, 16, device=DEV)
    gw, gb = _wg_run(0, 16, 16, x, dy, True)
    assert bool((gw == 0).all()) and bool((gb == 0).all())
    gw, gb = _wg_run(0, 16, 16, x, dy, False)
    assert bool((gw == 0).all())
    big = torch.zeros(8, 512, device=DEV)
    ws = torch.full((1024 * 160 * 256,), NAN, device=DEV)  # what the largest shape that is served with a bias asks for
    assert int(lib.mssvt_linear_wgrad_workspace_floats(8, 144, 256)) == ws.numel()
    dw, db = torch.full((512 * 512,), SENT, device=DEV), torch.full((512,), SENT, device=DEV)

    def call(cin, cout, X=big, DY=big, DW=dw, DB=db, WS=ws, M=8):
        return lib.mssvt_linear_wgrad(M, cin, cout, p(X), p(DY), p(DW), p(DB), p(WS), st)
    refused = {"Cin % 4": (call(18, 16), BADARG), "Cout % 4": (call(16, 18), BADARG), "X": (call(16, 16, X=None), BADARG),
               "dY": (call(16, 16, DY=None), BADARG), "dW": (call(16, 16, DW=None), BADARG), "ws": (call(16, 16, WS=None), BADARG),
               "M < 0": (call(16, 16, M=-1), BADARG), "176 tiles": (call(160, 256), TOOLARGE), "161 tiles": (call(352, 112), TOOLARGE),
               "no bias, 176": (call(176, 256, DB=None), TOOLARGE), "no bias, 161": (call(368, 112, DB=None), TOOLARGE)}
    for what, (got, want) in refused.items():
        assert got == want, what
    torch.cuda.synchronize()
    assert bool((dw == SENT).all()) and bool((db == SENT).all()) and bool(torch.isnan(ws).all())
    # the limit's other side: 160 tiles are served (exactly, on integers), with the bias column and one Cin tile further without
    g = torch.Generator().manual_seed(9)
    for cout, cin, with_db in ((256, 144, True), (160, 240, True), (256, 160, False), (112, 352, False)):
        xi, dyi = torch.randint(-3, 4, (81, cin), generator=g).float(), torch.randint(-3, 4, (81, cout), generator=g).float()
        want = ref.wgrad_ref(xi, dyi)
        gw, gb = _wg_run(81, cin, cout, xi.to(DEV), dyi.to(DEV), with_db)
        assert torch.equal(gw.cpu().double(), want[0]) and (gb is None or torch.equal(gb.cpu().double(), want[1]))
    for cout, cin in [(256, 144), (256, 160), (112, 352), (160, 240), (16, 18), (18, 16), (64, 64), (256, 256), (512, 64), (4, 4)]:
        assert (call(cin, cout) == OK) == train_path.wgrad_supported(cin, cout), (cout, cin)
    torch.cuda.synchronize()


@pytest.mark.parametrize("cout,cin,M", [(64, 64, 576), (20, 36, 513), (256, 144, 81)])
def test_wgrad_is_bit_identical_across_calls_and_streams(cout, cin, M):
    c = _wg_case(cout, cin)
    x, dy = c.d.xr[:M].contiguous(), c.d.dyr[:M].contiguous()
    a = _wg_run(M, cin, cout, x, dy, True)
    junk = _junk()
    b = _wg_run(M, cin, cout, x, dy, True)
    s = _on_second_stream(lambda: _wg_run(M, cin, cout, x, dy, True))
    for other in (b, s):
        assert _same_bits(a[0], other[0]) and _same_bits(a[1], other[1])
    del junk


# ---------------------------------------------------------------------------------------------------------
# b. mssvt_linear_rows / mssvt_linear_rows_h
# ---------------------------------------------------------------------------------------------------------

LR_SHAPES = [(64, 64), (64, 128), (128, 64), (128, 128)]  # (K, N): k_linear_rows<K, N / 16>
LH_SHAPES = LR_SHAPES + [(128, 256), (256, 128)]  # k_linear_rows_h<K, N>: KS = K / 32 <= 4 and the K = 256 form
LIN = [("mssvt_linear_rows", K, N) for K, N in LR_SHAPES] + [("mssvt_linear_rows_h", K, N) for K, N in LH_SHAPES]
LIN_ROWS = (1, 15, 16, 17, 31, 33, 127, 128, 129, 255, 256, 257)
X_PAD, X_C0, Y_PAD, Y_C0 = 8, 4, 12, 8  # X rows K + 8 wide, the columns at 4; Y rows N + 12 wide, the columns at 8, one row down


def _waves(name, K):
    return 8 if name == "mssvt_linear_rows" or K > 128 else 16  # LR_WAVES, LH_WAVES_OF(K)


def _x_wide(x):
    wide = torch.full((x.shape[0], x.shape[1] + X_PAD), 1e30, device=DEV)  # (a read outside the columns wrecks the sum)
    wide[:, X_C0:X_C0 + x.shape[1]] = x
    return wide


def _lin_run(name, M, K, N, xw, w, transpose_w, b, relu, scale, stream=None):
    """Strided call: X a column slice of `xw`, Y a column slice one row down in a sentinel tensor of M + 3 rows."""
    assert xw.shape == (M, K + X_PAD)  # the kernel reads M rows of K columns from column X_C0 on
    yw = torch.full((M + 3, N + Y_PAD), SENT, device=DEV)
    yw[1:M + 1, Y_C0:Y_C0 + N] = NAN
    _lib.call(name, M, K, N, xw.data_ptr() + 4 * X_C0, xw.stride(0), _lib.ptr(w), transpose_w, _lib.ptr(b), relu, scale,
              yw.data_ptr() + 4 * (yw.stride(0) + Y_C0), yw.stride(0), _lib.stream() if stream is None else stream)
    y = yw[1:M + 1, Y_C0:Y_C0 + N].clone()
    yw[1:M + 1, Y_C0:Y_C0 + N] = SENT
    assert bool((yw == SENT).all()), "Y was written outside rows [0, M) x columns [0, N)"
    return y


@functools.lru_cache(maxsize=None)
def _lin_case(K, N, transpose_w):
    g = torch.Generator().manual_seed(100 * K + N + transpose_w)
    M = max(LIN_ROWS)
    c = types.SimpleNamespace(K=K, N=N)
    c.pw2 = torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float())
    c.xi = torch.randint(-3, 4, (M, K), generator=g).float() * c.pw2  # integers times a power of two per row
    c.wi = torch.randint(-2, 3, (K, N) if transpose_w else (N, K), generator=g).float()
    c.bi = torch.randint(-3, 4, (N,), generator=g).float()
    c.xr = _scaled_rows(M, K, g)
    c.wr = torch.randn((K, N) if transpose_w else (N, K), generator=g) / K ** 0.5
    c.br = torch.randn(N, generator=g)
    c.d = types.SimpleNamespace(xi=_x_wide(c.xi.to(DEV)), xr=_x_wide(c.xr.to(DEV)), wi=c.wi.to(DEV), bi=c.bi.to(DEV),
                                wr=c.wr.to(DEV), br=c.br.to(DEV))
    return c


@pytest.mark.parametrize("transpose_w", [0, 1])
@pytest.mark.parametrize("name,K,N", LIN)
def test_linear_rows_every_form_strided(name, K, N, transpose_w):
    """bias x relu x out_scale at every M of LIN_ROWS, X and Y column slices of wider tensors: exact on integer
    operands, inside the derived bound on random ones; nothing outside Y's rows and columns is written."""
    c = _lin_case(K, N, transpose_w)
    split = name.endswith("_h")
    for bias in (True, False):
        for relu in (0, 1):
            for scale in (1.0, 0.25):
                yi, mi = ref.linear_ref(c.xi, c.wi, transpose_w, c.bi if bias else None, relu, scale)
                assert float((mi / c.pw2.clamp(max=1.0).double()).max()) < 2 ** 24  # in units of the row's last place
                yr, mr = ref.linear_ref(c.xr, c.wr, transpose_w, c.br if bias else None, relu, scale)
                lim = ref.linear_h_bound(c.xr, c.wr, transpose_w, mr, scale) if split else ref.linear_bound(K, mr, scale)
                worst = 0.0
                for M in LIN_ROWS:
                    got = _lin_run(name, M, K, N, c.d.xi[:M], c.d.wi, transpose_w, c.d.bi if bias else None, relu, scale)
                    assert torch.equal(got.cpu().double(), yi[:M]), ("exact", M, bias, relu, scale)
                    got = _lin_run(name, M, K, N, c.d.xr[:M], c.d.wr, transpose_w, c.d.br if bias else None, relu, scale)
                    err = (got.cpu().double() - yr[:M]).abs()
                    worst = max(worst, float((err / lim[:M]).max()))
                    assert bool((err <= lim[:M]).all()), ("bounded", M, bias, relu, scale, worst)
                print("%s (%d, %d) t%d b%d r%d s%g: worst |err| / bound = %.3f" % (name, K, N, transpose_w, bias, relu, scale, worst))


@pytest.mark.parametrize("name,K,N", LIN)
def test_linear_rows_compact_operands_give_the_strided_bits(name, K, N):
    c = _lin_case(K, N, 0)
    M = 129
    a = _lin_run(name, M, K, N, c.d.xr[:M], c.d.wr, 0, c.d.br, 1, 0.25)
    x, y = c.xr[:M].to(DEV), torch.full((M, N), NAN, device=DEV)
    _lib.call(name, M, K, N, _lib.ptr(x), K, _lib.ptr(c.d.wr), 0, _lib.ptr(c.d.br), 1, 0.25, _lib.ptr(y), N, _lib.stream())
    assert _same_bits(a, y)


@pytest.mark.parametrize("name,K,N", LIN)
def test_linear_rows_second_round_of_the_persistent_loop(name, K, N):
    """The first M at which a wave takes a second tile (grid = one workgroup per CU): cus 16 waves rows + 1, + 16, + 17.
    Exact operands; both weight layouts."""
    base = _cus() * 16 * _waves(name, K)
    g = torch.Generator().manual_seed(K + N)
    Mx = base + 17
    x = torch.randint(-3, 4, (Mx, K), generator=g, dtype=torch.float32) * torch.exp2(torch.randint(-8, 9, (Mx, 1), generator=g).float())
    b = torch.randint(-3, 4, (N,), generator=g).float()
    xw, bd = _x_wide(x.to(DEV)), b.to(DEV)
    for transpose_w in (0, 1):
        w = torch.randint(-2, 3, (K, N) if transpose_w else (N, K), generator=g).float()
        want, _ = ref.linear_ref(x, w, transpose_w, b, 1, 0.25)
        for M in (base + 1, base + 16, base + 17):
            got = _lin_run(name, M, K, N, xw[:M], w.to(DEV), transpose_w, bd, 1, 0.25)
            bad = (got.cpu().double() != want[:M]).any(1).nonzero().flatten()
            assert bad.numel() == 0, ("rows differ", M, bad[:8].tolist())


@pytest.mark.parametrize("name", ["mssvt_linear_rows", "mssvt_linear_rows_h"])
def test_linear_rows_status_codes(name):
    """BADARG: ldx < K, ldy < N, ldx & 3, a NULL pointer, M < 0; for the _h form also ldy & 3 and out_scale == 0.
    TOOLARGE: a (K, N) the kernel has no instantiation for; _supported() answers the same.  A refused call leaves Y alone."""
    lib, st = _lib.lib(), _lib.stream()
    fn, sup = getattr(lib, name), getattr(lib, name + "_supported")
    split = name.endswith("_h")
    x, w, b = torch.ones(16, 520, device=DEV), torch.ones(256 * 256, device=DEV), torch.ones(256, device=DEV)
    y = torch.full((16, 520), SENT, device=DEV)

    def call(K=64, N=64, X=x, W=w, Y=y, ldx=520, ldy=520, scale=1.0, M=16):
        return fn(M, K, N, _lib.ptr(X), ldx, _lib.ptr(W), 0, _lib.ptr(b), 0, scale, _lib.ptr(Y), ldy, st)
    refused = {"ldx < K": call(ldx=60), "ldy < N": call(ldy=60), "ldx & 3": call(ldx=66), "X": call(X=None), "W": call(W=None),
               "Y": call(Y=None), "M < 0": call(M=-1)}
    if split:
        refused.update({"ldy & 3": call(ldy=66), "out_scale == 0": call(scale=0.0)})
    for what, got in refused.items():
        assert got == BADARG, what
    for K in (32, 64, 128, 256):
        for N in (32, 64, 128, 256):
            ok = (K, N) in (LH_SHAPES if split else LR_SHAPES)
            assert sup(K, N) == (1 if ok else 0), (K, N)
            if not ok:
                assert call(K=K, N=N) == TOOLARGE, (K, N)
    assert call(M=0) == OK
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
    assert call() == OK
    torch.cuda.synchronize()
    assert bool((y[:, :64] == 65.0).all()) and bool((y[:, 64:] == SENT).all())


@pytest.mark.parametrize("transpose_w", [0, 1])
@pytest.mark.parametrize("K,N", LH_SHAPES)
def test_split_fp16_rows_outside_the_normal_range(K, N, transpose_w):
    """One 16-row tile whose rows 0 .. 5 are: all zero, all subnormal, largest value 2^126, largest value in
    [2^127, FLT_MAX], holding +inf, holding NaN.  pow2_norm (csrc/split_f16.hip.h) normalises a row whose largest
    exponent is 1 .. 254; a zero or subnormal row passes unscaled (its fp16 halves are 0: the bias, off by at most
    K 2^-126 max |W|); a NaN does not take part in the row's maximum and an inf row passes unscaled: both come out
    non-finite.  Every other row is inside its bound."""
    g = torch.Generator().manual_seed(K * 3 + N + transpose_w)
    M = 16
    x = _scaled_rows(M, K, g)
    x[0] = 0.0
    x[1] = torch.randint(-(2 ** 22), 2 ** 22, (K,), generator=g).float() * 2.0 ** -149
    x[2] = (torch.rand(K, generator=g) * 2 - 1) * 2.0 ** 126
    x[2, K // 3] = 2.0 ** 126
    x[3] = (torch.rand(K, generator=g) * 2 - 1) * 2.0 ** 127
    x[3, K // 2] = -1.7 * 2.0 ** 127
    x[3, 5] = ref.FLT_MAX
    x[4, 7] = float("inf")
    x[5, K - 1] = NAN
    assert float(x[1].abs().max()) < 2.0 ** -126 and float(x[1].abs().max()) > 0 and bool(torch.isfinite(x[3]).all())
    w = (torch.rand((K, N) if transpose_w else (N, K), generator=g) * 2 - 1) / K  # sum_k |w| < 1: the 2^126 row stays finite
    b = torch.randn(N, generator=g)
    got = _lin_run("mssvt_linear_rows_h", M, K, N, _x_wide(x.to(DEV)), w.to(DEV), transpose_w, b.to(DEV), 0, 1.0).cpu()
    fin = [0, 1, 2, 3] + list(range(6, M))
    want, mag = ref.linear_ref(x[fin], w, transpose_w, b, 0, 1.0)
    lim = ref.linear_h_bound(x[fin], w, transpose_w, mag, 1.0)
    lim[1] += K * 2.0 ** -126 * float(w.abs().max())
    err = (got[fin].double() - want).abs()
    held = want.abs() + lim <= ref.FLT_MAX  # the float64 result is a float32
    assert bool(held[[0, 1, 2] + list(range(4, len(fin)))].all()) and int(held[3].sum()) >= N // 2
    assert torch.equal(got[0], b)
    for r, what in ((1, "subnormal row"), (2, "2^126 row"), (3, "[2^127, FLT_MAX] row")):
        print("%s: worst |err| / bound = %.3f" % (what, float((err[r] / lim[r])[held[r]].max())))
        assert bool((err[r] <= lim[r])[held[r]].all()), what
    _inside(got[6:], want[4:], lim[4:], "mssvt_linear_rows_h (%d, %d) rows beside the extreme ones" % (K, N))
    assert not bool(torch.isfinite(got[4]).any()) and not bool(torch.isfinite(got[5]).any())


@pytest.mark.parametrize("name,K,N", LIN)
def test_linear_rows_bit_identical_across_calls_and_streams(name, K, N):
    c = _lin_case(K, N, 1)
    M = 257
    run = lambda: _lin_run(name, M, K, N, c.d.xr[:M], c.d.wr, 1, c.d.br, 0, 0.25)
    a = run()
    junk = _junk()
    b = run()
    s = _on_second_stream(run)
    assert _same_bits(a, b) and _same_bits(a, s)
    del junk


# ---------------------------------------------------------------------------------------------------------
# c. mssvt_pair_attention_fwd / _bwd
# ---------------------------------------------------------------------------------------------------------

# (cg, hd) -> k_pair_attn_*<CPL = 1 + (cg > 64), hd>.  CPL = 1: cg = hd, a cg between hd and 64 (hd = 32 divides none; hd = 64 has
# cg = 64 alone), cg = 64.  CPL = 2: cg = 128 and the smallest cg > 64 that hd divides: 4, 8, 16, 32 lanes of the second pass
# work, the others idle (hd = 64: cg = 128 alone).
PA_SHAPES = [(4, 4), (20, 4), (64, 4), (8, 8), (40, 8), (64, 8), (16, 16), (48, 16), (64, 16), (32, 32), (64, 32), (64, 64),
             (128, 4), (68, 4), (128, 8), (72, 8), (128, 16), (80, 16), (128, 32), (96, 32), (128, 64)]
ROW = 2  # rows of 1e30 before and after q, kv, dO


def test_attention_shapes_reach_every_instantiation():
    inst = {(1 + (cg > 64), hd) for cg, hd in PA_SHAPES}
    assert inst == {(c, h) for c in (1, 2) for h in (4, 8, 16, 32, 64)}
    assert all(cg % hd == 0 for cg, hd in PA_SHAPES)


def _embed(t):
    """t between ROW rows of 1e30; returns (the allocation, the address of t's first row)."""
    wide = torch.full((t.shape[0] + 2 * ROW, t.shape[1]), 1e30, device=DEV)
    wide[ROW:ROW + t.shape[0]] = t
    return wide, wide.data_ptr() + 4 * ROW * t.shape[1]


class _PaRun:
    """One case on the GPU: O, lse, dq, dkv are NaN-filled pieces of ONE sentinel-filled allocation, G sentinels before,
    between and after them; q, kv, dO lie between rows of 1e30."""

    def __init__(self, wins, q, kv, dO, heads, hd):
        self.heads, self.hd, self.cg = heads, hd, heads * hd
        self.R, self.Kn, self.nw = q.shape[0], kv.shape[0], wins[0].numel()
        self.wins = [a.int().to(DEV) for a in wins]
        self.keep = [_embed(t.to(DEV)) for t in (q, kv, dO)]
        sizes = dict(O=self.R * self.cg, lse=self.R * heads, dq=self.R * self.cg, dkv=self.Kn * 2 * self.cg)
        self.at, n = {}, G
        for k, v in sizes.items():
            self.at[k] = (n, v)
            n += v + G
        self.total = n
        self.fresh()

    def fresh(self):
        self.buf = torch.full((self.total,), SENT, device=DEV)
        for o, n in self.at.values():
            self.buf[o:o + n] = NAN

    def ptr(self, k):
        return self.buf.data_ptr() + 4 * self.at[k][0]

    def get(self, k):
        o, n = self.at[k]
        return self.buf[o:o + n].clone().view(self.R if k != "dkv" else self.Kn, -1)

    def put(self, k, t):
        o, n = self.at[k]
        self.buf[o:o + n] = t.to(DEV).float().reshape(-1)

    def guards_intact(self, untouched=()):
        out = self.buf.clone()
        for k, (o, n) in self.at.items():
            if k in untouched:
                assert bool(torch.isnan(out[o:o + n]).all()), k + " was written"
            out[o:o + n] = SENT
        assert bool((out == SENT).all()), "a word outside O / lse / dq / dkv changed"

    def fwd(self, stream=None):
        _lib.call("mssvt_pair_attention_fwd", self.nw, self.cg, self.heads, self.hd, *[_lib.ptr(a) for a in self.wins],
                  self.keep[0][1], self.keep[1][1], self.ptr("O"), self.ptr("lse"), _lib.stream() if stream is None else stream)

    def bwd(self, with_dq=True, stream=None):
        _lib.call("mssvt_pair_attention_bwd", self.nw, self.cg, self.heads, self.hd, *[_lib.ptr(a) for a in self.wins],
                  self.keep[0][1], self.keep[1][1], self.ptr("O"), self.ptr("lse"), self.keep[2][1],
                  self.ptr("dq") if with_dq else None, self.ptr("dkv"), _lib.stream() if stream is None else stream)


def _pa_bounded(cg, hd, kind, pairs=None, seed=0):
    heads = cg // hd
    wins, q, kv, dO = ref.attn_operands(1000 * cg + hd + seed, heads, hd, kind, pairs)
    r = ref.attn_ref(wins, q, kv, dO, heads, hd)
    run = _PaRun(wins, q, kv, dO, heads, hd)
    run.fwd()
    run.guards_intact(untouched=("dq", "dkv"))
    tag = "(cg %d, hd %d, %s)" % (cg, hd, kind)
    _inside(run.get("O"), r["O"], r["bO"], "mssvt_pair_attention_fwd O " + tag)
    _inside(run.get("lse"), r["lse"], r["blse"], "mssvt_pair_attention_fwd lse " + tag)
    # the backward alone: handed the float32 rounding of the statement's O and lse, held to the statement on those
    O32, lse32 = r["O"].float(), r["lse"].float()
    rb = ref.attn_ref(wins, q, kv, dO, heads, hd, O_in=O32, lse_in=lse32)
    run.fresh()
    run.put("O", O32)
    run.put("lse", lse32)
    run.bwd()
    run.guards_intact()
    assert _same_bits(run.get("O"), O32.to(DEV)) and _same_bits(run.get("lse"), lse32.to(DEV))
    _inside(run.get("dq"), rb["dq"], rb["bdq"], "mssvt_pair_attention_bwd dq " + tag)
    _inside(run.get("dkv"), rb["dkv"], rb["bdkv"], "mssvt_pair_attention_bwd dkv " + tag)
    return run


@pytest.mark.parametrize("cg,hd", PA_SHAPES)
def test_attention_every_instantiation_on_the_window_grid(cg, hd):
    """All 72 (nq, nk) pairs of ref.NQS x ref.NKS (+ one: 73 windows, the last workgroup has one), shuffled, rows out of
    order; scores up to about 60."""
    _pa_bounded(cg, hd, "hot")


@pytest.mark.parametrize("cg,hd", PA_SHAPES)
def test_attention_exact_degenerate_windows(cg, hd):
    """Integer operands.  nk = 1: O = v, lse = the score, dq = dk = 0, dv = the sum of the window's dO rows, all exactly.
    nq = 0: the window's dkv rows are 0.  nk = 0: O, lse, dq rows are 0."""
    heads = cg // hd
    wins, q, kv, dO = ref.attn_operands(77 * cg + hd, heads, hd, "int")
    run = _PaRun(wins, q, kv, dO, heads, hd)
    run.fwd()
    run.bwd()  # on the kernel's own O and lse
    run.guards_intact()
    O, lse, dq, dkv = (run.get(k).cpu() for k in ("O", "lse", "dq", "dkv"))
    assert bool(torch.isfinite(O).all() and torch.isfinite(lse).all() and torch.isfinite(dq).all() and torch.isfinite(dkv).all())
    seen = set()
    for qo, nq, ko, nk in zip(*[a.tolist() for a in wins]):
        rows, keys = slice(qo, qo + nq), slice(ko, ko + nk)
        if nk == 0:
            assert not bool(O[rows].any()) and not bool(lse[rows].any()) and not bool(dq[rows].any())
            seen.add("nk0")
        if nq == 0:
            assert not bool(dkv[keys].any())
            seen.add("nq0")
        if nk == 1 and nq > 0:
            k, v = kv[ko, :cg], kv[ko, cg:]
            assert torch.equal(_bits(O[rows]), _bits(v.expand(nq, cg)))
            s = (q[rows] * k).view(nq, heads, hd).sum(-1)
            assert float(s.abs().max()) < 2 ** 24 and torch.equal(lse[rows], s)  # (the value: a zero score's sign is the add order's)
            assert not bool(dq[rows].any()) and not bool(dkv[ko, :cg].any())
            assert torch.equal(dkv[ko, cg:], dO[rows].sum(0))
            seen.add("nk1")
    assert seen == {"nk0", "nq0", "nk1"}


@pytest.mark.parametrize("cg,hd", [(64, 16), (96, 32), (20, 4)])
@pytest.mark.parametrize("kind", ["same", "dominant", "grid"])
def test_attention_identical_and_dominant_keys(cg, hd, kind):
    _pa_bounded(cg, hd, kind)


@pytest.mark.parametrize("cg,hd", [(64, 16), (96, 32)])
@pytest.mark.parametrize("nw", [1, 4, 5])
def test_attention_window_counts_around_one_workgroup(cg, hd, nw):
    _pa_bounded(cg, hd, "hot", pairs=[(33, 33), (9, 17), (8, 4), (17, 5), (1, 1)][:nw], seed=nw)


@pytest.mark.parametrize("cg,hd", [(64, 16), (128, 16), (72, 8)])
def test_attention_other_forms_and_run_to_run_bits(cg, hd):
    """dq == NULL: the same dkv bits, nothing else written.  nw = 0: OK, nothing written.  Two calls and a second
    stream: the same bits."""
    heads = cg // hd
    wins, q, kv, dO = ref.attn_operands(5 * cg + hd, heads, hd, "hot")
    run = _PaRun(wins, q, kv, dO, heads, hd)
    run.fwd()
    run.bwd()
    a = {k: run.get(k) for k in ("O", "lse", "dq", "dkv")}
    junk = _junk()
    again = _PaRun(wins, q, kv, dO, heads, hd)
    again.fwd()
    again.bwd()
    other = _PaRun(wins, q, kv, dO, heads, hd)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        other.fwd()
        other.bwd()
    st.synchronize()
    for r in (again, other):
        for k in a:
            assert _same_bits(a[k], r.get(k)), k
        r.guards_intact()
    only = _PaRun(wins, q, kv, dO, heads, hd)
    only.put("O", a["O"])
    only.put("lse", a["lse"])
    only.bwd(with_dq=False)
    only.guards_intact(untouched=("dq",))
    assert _same_bits(only.get("dkv"), a["dkv"]) and _same_bits(only.get("O"), a["O"]) and _same_bits(only.get("lse"), a["lse"])
    none = _PaRun(wins, q, kv, dO, heads, hd)
    none.nw = 0
    none.fwd()
    none.bwd()
    none.guards_intact(untouched=("O", "lse", "dq", "dkv"))
    del junk


def test_attention_refusals():
    """BADARG: cg > 128, heads hd != cg, hd not in {4, 8, 16, 32, 64}, a NULL window array; nothing is written."""
    heads, hd = 4, 16
    wins, q, kv, dO = ref.attn_operands(1, heads, hd, "grid", [(8, 4), (1, 1), (9, 5)])
    run = _PaRun(wins, q, kv, dO, heads, hd)
    lib, st = _lib.lib(), _lib.stream()
    w = [_lib.ptr(a) for a in run.wins]

    def fwd(cg=64, heads=4, hd=16, wins=w, nw=3):
        return lib.mssvt_pair_attention_fwd(nw, cg, heads, hd, *wins, run.keep[0][1], run.keep[1][1], run.ptr("O"), run.ptr("lse"), st)

    def bwd(cg=64, heads=4, hd=16, wins=w, nw=3):
        return lib.mssvt_pair_attention_bwd(nw, cg, heads, hd, *wins, run.keep[0][1], run.keep[1][1], run.ptr("O"), run.ptr("lse"),
                                            run.keep[2][1], run.ptr("dq"), run.ptr("dkv"), st)
    for f in (fwd, bwd):
        refused = {"cg > 128": f(cg=144, heads=9), "heads hd != cg": f(heads=3), "hd = 2": f(heads=32, hd=2), "hd = 12": f(cg=48, heads=4, hd=12),
                   "hd = 128": f(cg=128, heads=1, hd=128), "nw < 0": f(nw=-1)}
        for i in range(4):
            refused["NULL window array %d" % i] = f(wins=w[:i] + [None] + w[i + 1:])
        for what, got in refused.items():
            assert got == BADARG, (f.__name__, what)
    torch.cuda.synchronize()
    run.guards_intact(untouched=("O", "lse", "dq", "dkv"))
