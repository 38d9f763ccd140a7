"""The two ends of a k_ffn_ws launch (csrc/ffn.hip): the head, which orders its loads by where the row count lives, and the
peeled tail, in which a workgroup's last tile runs GEMM2 and D alone.

tests/test_ffn_forms_gpu.py pins every form to float64 at the pipeline's regimes; this file aims at what the head / tail
split can break, with that file's cases, reference and bounds (check_outputs):
  * row counts that put workgroups with zero, one and two tiles side by side (tiles = 1, 2, G - 1, G, G + 1, 2G, 2G + 1, G
    the launch grid from the device's CU count), n = 1, 15, 16, 17, and both sides of the XCD deal (8G - 1, 8G, 8G + 9 tiles);
  * every instantiation -- table / plain / owner input, with and without the next LayerNorm, with and without the y store,
    packed fragments and fp32 weights split in the head -- with the row count on the host and on the device (0 rows, and a
    count below the capacity);
  * rows at and beyond n up to the capacity keep NaN canaries in y and y_norm: the tail no longer repeats a tile whose
    clamped duplicates store equal values, so a tail that runs a tile too many or too few shows here;
  * the same input rows give the same bits as the first tile of a workgroup (head), a steady tile (loop), its last tile (tail)
    and its only tile (head straight into the tail);
  * two launches give the same bits.
"""
import pytest
import torch

from tests.test_ffn_forms_gpu import DEV, FORMS, SHAPES, WS_FORMS, check_outputs, grid_of, on_gpu, ws_regime

pytestmark = pytest.mark.gpu

MAIN = (128, 256)
# name -> rows(G): the last tile is partial wherever the count is given in tiles
TILES = {"1t": lambda G: 1, "2t": lambda G: 2, "G-1": lambda G: G - 1, "G": lambda G: G, "G+1": lambda G: G + 1,
         "2G": lambda G: 2 * G, "2G+1": lambda G: 2 * G + 1, "8G-1": lambda G: 8 * G - 1, "8G": lambda G: 8 * G,
         "8G+9": lambda G: 8 * G + 9}
ROWS = {"n1": 1, "n15": 15, "n16": 16, "n17": 17}


def rows_of(C, FF, count):
    return ROWS[count] if count in ROWS else 16 * TILES[count](grid_of("ws", C, FF)) - 5


def nan_buffers(g, rows):
    c = g.case
    return (torch.full((rows, c.C), float("nan"), dtype=torch.float32, device=DEV),
            torch.full((rows, c.C), float("nan"), dtype=torch.float32, device=DEV), None)


def check_canaries_and_bits(g, form, first, cap, n_dev=None):
    """A second launch into NaN-filled buffers of `cap` + 32 rows: rows [n, cap + 32) stay NaN in both outputs, rows [0, n)
    carry the bits of `first`."""
    c = g.case
    r = g.launch(form, n_rows=cap, n_dev=n_dev, out=nan_buffers(g, cap + 32))
    assert r.st == 0
    for name, got, ref, on in (("y", r.y, first.y, form.store_y), ("y_norm", r.yn, first.yn, form.norm)):
        if not on:
            assert bool(torch.isnan(got).all()), (form.id, name, "written without being asked for")
            continue
        assert bool(torch.isnan(got[c.n:]).all()), (form.id, name, "a row at or beyond n was written")
        assert torch.equal(got[:c.n], ref[:c.n]), (form.id, name, "two launches differ")


@pytest.mark.parametrize("count", list(ROWS) + list(TILES))
def test_row_counts_vs_float64_canaries_and_repeat(count):
    C, FF = MAIN
    G, n = grid_of("ws", C, FF), rows_of(C, FF, count)
    grid, per_wg, dealt = ws_regime(n, G)
    if count in TILES:  # what the count is for
        tiles = TILES[count](G)
        assert grid == min(G, tiles) and dealt == (tiles >= 8 * G)
        assert per_wg == {"1t": 1, "2t": 1, "G-1": 1, "G": 1, "G+1": 2, "2G": 2, "2G+1": 3, "8G-1": 8, "8G": 8, "8G+9": 9}[count]
    for fid in ("ws-table-norm-packed", "ws-plain-nonorm-packed"):  # the Block form and the CompressBlock form of the frame
        form = FORMS[fid]
        g = on_gpu(C, FF, n, form.source)
        first = g.run(form)
        check_outputs(g, form, first, "%dx%d %s" % (C, FF, count))
        check_canaries_and_bits(g, form, first, n)


def _form_params():
    out = []
    for C, FF in SHAPES:
        for f in WS_FORMS:
            for count in (("1t", "G+1", "2G+1") if (C, FF) == MAIN else ("G+1",)):
                out.append(pytest.param(C, FF, count, f.id, id="%dx%d-%s-%s" % (C, FF, count, f.id)))
    return out


@pytest.mark.parametrize("C,FF,count,form", _form_params())
def test_every_instantiation_host_count(C, FF, count, form):
    form = FORMS[form]
    n = rows_of(C, FF, count)
    g = on_gpu(C, FF, n, form.source)
    first = g.run(form)
    check_outputs(g, form, first, "%dx%d %s" % (C, FF, count))
    check_canaries_and_bits(g, form, first, n)


def _dev_params():
    out = []
    for C, FF in SHAPES:
        for f in WS_FORMS:
            if (C, FF) != MAIN and f.id != "ws-plain-nonorm-packed":
                continue
            for k in ("zero", "below"):
                out.append(pytest.param(C, FF, k, f.id, id="%dx%d-%s-%s" % (C, FF, k, f.id)))
    return out


@pytest.mark.parametrize("C,FF,kind,form", _dev_params())
def test_every_instantiation_device_count(C, FF, kind, form):
    """The count on the device: the grid is sized by the capacity (2G + 1 tiles), the count leaves workgroups without a
    tile (zero: all of them), with one and with two."""
    form = FORMS[form]
    G = grid_of("ws", C, FF)
    cap = 16 * (2 * G + 1) - 5
    n = 0 if kind == "zero" else 16 * (G + G // 2) - 7
    g = on_gpu(C, FF, n, form.source, cap=cap)
    host = g.launch(form, n_rows=n) if n else None  # the same rows under a host count
    r = g.launch(form, n_rows=cap, n_dev=n)
    check_outputs(g, form, r, "%dx%d device count %s" % (C, FF, kind))
    if n:
        for got, ref, on in ((r.y, host.y, form.store_y), (r.yn, host.yn, form.norm)):
            assert not on or torch.equal(got[:n], ref[:n]), (form.id, "device and host count differ")
    check_canaries_and_bits(g, form, r, cap, n_dev=n)


@pytest.mark.parametrize("form", ["ws-table-norm-packed", "ws-plain-nonorm-packed", "ws-owner-norm-unpacked", "ws-table-noy"])
def test_same_rows_same_bits_in_first_steady_last_and_only_tile(form):
    """5 G tiles of rows; the G tiles [2G, 3G) are placed by the rows in front of and behind them (row pointers offset by
    r0, n_rows rows launched; round-robin dealing below 8 G tiles): workgroup b's tile 2G + b is its
      last of three (tail)            r0 = 0,      3G tiles        steady, third of five (loop)   r0 = 0,      5G tiles
      first of three (head)           r0 = 2G,     3G tiles        only tile (head -> tail)       r0 = 2G,     G tiles
      steady, second of three (loop)  r0 = G,      3G tiles"""
    C, FF = MAIN
    form = FORMS[form]
    G = grid_of("ws", C, FF)
    T = 16 * G  # rows of G tiles
    g = on_gpu(C, FF, 5 * T, form.source)
    outs = {}
    for name, r0, tiles in (("last", 0, 3), ("steady3of5", 0, 5), ("first", 2, 3), ("only", 2, 1), ("steady2of3", 1, 3)):
        assert ws_regime(tiles * T, G) == (G, tiles, False)
        r = g.launch(form, r0=r0 * T, n_rows=tiles * T, out=g.buffers(form, 5 * T + 32))  # whole-case buffers: written at row r0
        assert r.st == 0
        outs[name] = (r.y[2 * T:3 * T].clone(), r.yn[2 * T:3 * T].clone())
    y0, yn0 = outs["steady3of5"]
    assert (not form.store_y or bool(torch.isfinite(y0).all())) and (not form.norm or bool(torch.isfinite(yn0).all()))
    for name, (y, yn) in outs.items():
        if form.store_y:
            assert torch.equal(y, y0), (form.id, name, "y differs from the steady tile's")
        if form.norm:
            assert torch.equal(yn, yn0), (form.id, name, "y_norm differs from the steady tile's")
