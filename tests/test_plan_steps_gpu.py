"""The step lists of the paired window launch and the flag they are built from.

  * mssvt_plan_order_steps on hand-made nq_valid and flags (no plan kernel): the lists against the statement of their
    contract (tests/kvh_pairs_ref.py: every active window in exactly one step, pairs = two distinct unflagged windows of one
    count, heaviest first, at most one unflagged window per count alone, nothing written at or behind num_steps), and perm /
    q_off / rows / counts against mssvt_plan_order's contract as the plain call -- with one and with several workgroups per
    list, all counts equal (one bucket), odd sub-buckets, flags all set / all clear / mixed, counts above the 256-key clamp, and
    the capacity at exactly the number of windows;
  * the flag itself: mssvt_window_plan_two_live on the hand-built levels of tests/test_window_plan_forms_gpu.py leaves every
    output of mssvt_window_plan_two_vox as the reference states it, and live1 / live2 equal the flag computed on the host from
    the kmeta the same launch wrote.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import kvh_pairs_ref as pr
from tests import test_window_plan_forms_gpu as F
from tests import window_plan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NG = 2


def _flags(kind, cap, seed):
    rng = np.random.default_rng(seed)
    if kind == "set":
        return [np.ones(cap, np.int32)] * NG
    if kind == "clear":
        return [np.zeros(cap, np.int32)] * NG
    return [(rng.random(cap) < p).astype(np.int32) for p in (0.1, 0.6)]


def _run(sets, flags, cap, rc, nw):
    """sets: [(nq_valid, qmeta bits, nq)].  Returns (plan-order outputs per set, steps[set][group], num_steps[set][group])."""
    from mssvt_amd import _lib
    lib, n = _lib.lib(), len(sets)
    full = F._full
    dev = [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b, _ in sets]
    live = [torch.from_numpy(f).to(DEV) for f in flags]
    num_wins = full((1,), nw)
    o = [dict(perm=full((cap,), -7), n_act=full((1,), -7), q_off=full((cap,), -7), meta=full((rc, 4), float("nan"), torch.float32),
              src=full((rc, 2), -7), n_rows=full((1,), -7)) for _ in range(n)]
    steps = [full((cap + 2, 2), -7) for _ in range(n * NG)]
    nst = [full((2,), -7) for _ in range(n * NG)]
    scratch = full((int(lib.mssvt_plan_order_steps_scratch_ints(n, NG)),), -7)
    pa = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    st = lib.mssvt_plan_order_steps(
        n, num_wins.data_ptr(), pa([d[0] for d in dev]), (ctypes.c_int * n)(*[s[2] for s in sets]), pa([d[1] for d in dev]), cap, rc,
        pa([x["perm"] for x in o]), pa([x["n_act"] for x in o]), pa([x["q_off"] for x in o]), pa([x["meta"] for x in o]),
        pa([x["src"] for x in o]), pa([x["n_rows"] for x in o]), NG, pa(live), pa(steps), pa(nst), scratch.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert st == 0
    outs = [{k: v.cpu().numpy() for k, v in x.items()} for x in o]
    return outs, [s.cpu().numpy() for s in steps], [t.cpu().numpy() for t in nst]


CASES = {
    # name: (cap, nw, [(pattern, nq)], flags)
    "one_workgroup": (1500, 1400, [("random", 6), ("random", 27)], "mixed"),
    "three_workgroups": (3 * 2048 + 100, 3 * 2048 + 100, [("random", 6), ("above256", 300)], "mixed"),  # capacity = windows
    "one_bucket": (2 * 2048 + 5, 2 * 2048 + 5, [("equal", 6)], "mixed"),
    "one_bucket_clear_odd": (2 * 2048 + 5, 2 * 2048 + 5, [("equal", 6)], "clear"),  # 4101 windows of one count: one alone
    "all_set": (2100, 2000, [("random", 6)], "set"),
    "all_clear": (2100, 2000, [("random", 6)], "clear"),
    "no_query": (300, 300, [("zero", 6)], "mixed"),
    "one_window": (8, 1, [("equal", 6)], "clear"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_step_lists_hold_their_contract(name):
    cap, nw, pats, fkind = CASES[name]
    sets = []
    for i, (pat, nq) in enumerate(pats):
        nqv, order = F._make_set(pat, cap, nq, 900 + i)
        sets.append((nqv, F._qmeta(nqv, order, 900 + i), nq))
    rc = max(int(max(s[0][:nw].sum() for s in sets)), 1)
    flags = _flags(fkind, cap, 77)
    G = F._groups(cap, rc)
    assert (G > 1) == (name in ("three_workgroups", "one_bucket", "one_bucket_clear_odd")), G
    outs, steps, nst = _run(sets, flags, cap, rc, nw)
    for i, (nqv, qm, nq) in enumerate(sets):
        x = outs[i]
        R.check_plan_order(nqv, nw, nq, qm, rc, x["perm"], x["n_act"][0], x["q_off"], x["n_rows"][0], x["src"], x["meta"].view(np.int32))
        for g in range(NG):
            s, n = steps[i * NG + g], nst[i * NG + g]
            assert n[1] == -7 and 0 <= n[0] <= cap
            pr.check_steps(nqv, flags[g], nw, s, int(n[0]), max_key=min(nq, 256))
            assert (s[n[0]:] == -7).all()  # nothing at or behind num_steps
            if fkind == "set":
                assert n[0] == x["n_act"][0] and (s[:n[0], 1] == -1).all()
            if name == "one_bucket_clear_odd":
                assert n[0] == (nw + 1) // 2 and int((s[:n[0], 1] < 0).sum()) == 1
            if fkind == "clear" and name != "one_window":
                assert n[0] < x["n_act"][0]
    if name == "one_window":
        assert [int(t[0]) for t in nst] == [1, 1] and steps[0][0].tolist() == [0, -1]


def _live_cases():
    return [n for n in sorted(F.CONFIGS) if F.CONFIGS[n].vox_ok and not F.CONFIGS[n].tall]


@pytest.mark.parametrize("name", _live_cases())
def test_upper_tile_flag_equals_the_flag_of_the_kmeta_the_launch_wrote(name):
    from mssvt_amd import _lib
    g = F.on_gpu(name)
    a = g.mode_args("ranked")
    out = g.buffers()
    for k in F.OUTPUTS:
        a[k] = out[k].data_ptr()
    out["vox_win"] = F._full((g.N,), -1)
    live = [F._full((g.cap,), -7) for _ in range(2)]
    st = _lib.lib().mssvt_window_plan_two_live(*[a[k] for k in F.NAMES], out["vox_win"].data_ptr(), live[0].data_ptr(),
                                               live[1].data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert st == 0
    g.check(out, "_two_live")  # every other output as without the flags
    for i, k in enumerate(("kmeta1", "kmeta2")):
        rows = out[k].view(torch.int32)[:g.nw, :, 3].cpu().numpy()
        want = pr.upper_live(rows)
        got = live[i].cpu().numpy()
        assert np.array_equal(got[:g.nw], want), k
        assert (got[g.nw:] == -7).all()
    print("\n%s: K = %d, nw = %d, flagged %s" % (name, g.cfg.K, g.nw, [int(x[:g.nw].sum()) for x in (live[0].cpu(), live[1].cpu())]))
