"""The step lists of the paired window launch (include/mssvt_hip.h: mssvt_plan_order_steps) as a statement of their
contract on numpy arrays, and the plan kernel's upper-tile flag restated from the kmeta it wrote.  No GPU here."""
import numpy as np


def upper_live(kmeta_rows):
    """(windows, K) int32 feature rows of a key scale (-1 = masked slot) -> per window 1 when a slot 16 .. K-1 holds a row."""
    return (np.asarray(kmeta_rows)[:, 16:] >= 0).any(1).astype(np.int32)


def check_steps(nq_valid, live, nw, steps, num_steps, max_key=256):
    """steps (cap, 2) / num_steps against the contract, for windows [0, nw) with flags `live`."""
    nqv = np.minimum(np.asarray(nq_valid)[:nw], max_key)
    live = np.asarray(live)[:nw]
    active = np.nonzero(nqv > 0)[0]
    s = np.asarray(steps).reshape(-1, 2)[:num_steps]
    a, b = s[:, 0], s[:, 1]
    # every active window in exactly one step, nothing else listed
    listed = np.concatenate([a, b[b >= 0]])
    assert np.all((listed >= 0) & (listed < nw))
    assert np.array_equal(np.sort(listed), active), (listed.size, active.size)
    assert np.all(b >= -1) and np.all(a >= 0)
    # a pair: two distinct windows of one count whose flag is clear
    pr = b >= 0
    assert np.all(a[pr] != b[pr])
    assert np.all(live[a[pr]] == 0) and np.all(live[b[pr]] == 0)
    assert np.array_equal(nqv[a[pr]], nqv[b[pr]])
    # heaviest first
    heavy = np.where(pr, np.maximum(nqv[a], nqv[np.maximum(b, 0)]), nqv[a])
    assert np.all(heavy[:-1] >= heavy[1:])
    # at most one pairable window of a count is alone
    alone = a[~pr]
    lone_pairable = nqv[alone[live[alone] == 0]]
    assert np.unique(lone_pairable).size == lone_pairable.size
    want = 0
    for n in np.unique(nqv[active]):
        c1 = int(((nqv == n) & (live == 0)).sum())
        want += (c1 + 1) // 2 + int(((nqv == n) & (live != 0)).sum())
    assert num_steps == want, (num_steps, want)
