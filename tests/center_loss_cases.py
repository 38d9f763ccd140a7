"""Generated inputs of tests/test_center_loss_gpu.py (TEST INFRASTRUCTURE ONLY), kept apart from it so that
tests/test_center_loss_ref_cpu.py can hold every one of them to its conditions without the library:
  * no logit has |x| in (9.0, 9.5): the clamp's edges sit at +-9.2102, and a one-ulp difference between two sigmoids must
    not flip a gradient between zero and non-zero;
  * at most 2 % of the logits are saturated (|x| >= 9.5), the planted ones included.
A case is a dict of numpy arrays: hm, heatmap (B, C, H, W) f32, maps [(B, c_k, H, W) f32] in HEAD_ORDER, target_boxes
(B, M, D + 1) f32 (the label column rides along, as in CenterHead's targets), inds / masks (B, M) i64, code_weights (D),
loc_weight; plus `planted`: flat indices into hm of the saturated logits put there on purpose."""
import numpy as np

SWEEP = 1024  # include/mssvt_hip.h MSSVT_CENTER_LOSS_SWEEP: elements a workgroup covers per grid-stride step
MAX_BLOCKS = 2048  # MSSVT_CENTER_LOSS_MAX_BLOCKS: the grid is min(ceil(n / SWEEP), MAX_BLOCKS)
CHANNELS = {8: (2, 1, 3, 2), 10: (2, 1, 3, 2, 2), 17: (2, 1, 3, 2, 9)}  # center, center_z, dim, rot[, vel]

# name -> (B, C, H, W, M, D), options
CASES = {
    "one_cell": ((1, 1, 1, 1, 1, 8), {}),
    "tail_only": ((1, 1, 5, 3, 4, 8), {}),
    "odd_n": ((2, 3, 33, 37, 20, 8), dict(plant=True)),
    "with_vel": ((3, 2, 64, 64, 500, 10), dict(plant=True)),
    "sweep_minus_1": ((1, 1, 3, 341, 8, 8), {}),  # n = SWEEP - 1
    "sweep": ((1, 1, 32, 32, 8, 8), {}),  # n = SWEEP: one workgroup, body only
    "sweep_plus_1": ((1, 1, 25, 41, 8, 8), {}),  # n = SWEEP + 1: a second workgroup for one element
    "stride_twice": ((1, 1, 12, 174763, 8, 8), {}),  # n = MAX_BLOCKS SWEEP + 4: the first float4 of a second grid-stride step
    "no_positives": ((2, 3, 33, 37, 20, 8), dict(positives="none")),
    "no_objects": ((2, 3, 33, 37, 20, 8), dict(masks="none", positives="none")),
    "one_empty_sample": ((3, 2, 17, 19, 12, 8), dict(empty_sample=1)),
    "two_on_a_cell": ((2, 2, 9, 7, 12, 8), dict(dup=2)),
    "three_on_a_cell": ((2, 2, 9, 7, 12, 8), dict(dup=3)),
    "all_on_a_cell": ((2, 2, 9, 7, 12, 8), dict(dup="all")),
    "poisoned_slots": ((2, 2, 9, 7, 12, 8), dict(poison=True)),
}
assert 3 * 341 == SWEEP - 1 and 32 * 32 == SWEEP and 25 * 41 == SWEEP + 1 and 12 * 174763 == MAX_BLOCKS * SWEEP + 4


def make_case(name):
    (B, C, H, W, M, D), opt = CASES[name]
    return generate(B, C, H, W, M, D, seed=sorted(CASES).index(name), **opt)


def generate(B, C, H, W, M, D, seed=0, plant=False, positives="some", masks="some", empty_sample=None, dup=0, poison=False):
    rng = np.random.default_rng(1000 + seed)
    HW = H * W
    hm = rng.normal(-2.19, 2.0, (B, C, H, W)).astype(np.float32)
    edge = (np.abs(hm) > 9.0) & (np.abs(hm) < 9.5)
    hm[edge] = np.sign(hm[edge]) * np.float32(8.75)  # clear of the clamp's edges
    # target heat map: mostly zero, Gaussian-like values below 1 on a tenth of the cells, exact ones at the objects
    heatmap = np.where(rng.random((B, C, H, W)) < 0.1, rng.random((B, C, H, W)) * 0.98, 0.0).astype(np.float32)
    maps = [rng.normal(0.0, 1.0, (B, c, H, W)).astype(np.float32) for c in CHANNELS[D]]
    target = rng.normal(0.0, 1.0, (B, M, D + 1)).astype(np.float32)
    target[:, :, D] = rng.integers(1, C + 1, (B, M))
    inds = rng.integers(0, HW, (B, M)).astype(np.int64)
    mask = np.zeros((B, M), np.int64)
    for b in range(B):
        k = int(rng.integers(1, M + 1))
        mask[b, :k] = 1
        if k > 2:
            mask[b, k // 2] = 0  # a masked slot among the unmasked ones
    if masks == "none":
        mask[:] = 0
    if empty_sample is not None:
        mask[empty_sample] = 0
    if dup:
        for b in range(B):
            js = np.arange(M) if dup == "all" else np.sort(rng.choice(M, size=dup + 1, replace=False))
            inds[b, js] = inds[b, js[0]]
            mask[b, js] = 1
            mask[b, js[len(js) // 2]] = 0  # one of them is masked out: it must not contribute
            if b == 0:  # sign(0) = 0: one duplicate's target equals the prediction in one code dimension
                target[0, js[-1], 0] = maps[0][0, 0].reshape(-1)[inds[0, js[-1]]]
    if poison:
        mask[:, :4] = np.array([1, 0, 1, 1])
        target[:, 1, :] = np.nan  # masked out: never read
        inds[:, 1] = 2 ** 40
        inds[0, 2] = HW  # unmasked and just outside the map: counts in num, contributes nothing
        inds[1, 2] = -1
    if positives != "none":
        flat = heatmap.reshape(B, C, HW)
        for b, j in zip(*np.nonzero(mask)):
            if 0 <= inds[b, j] < HW:
                flat[b, int(target[b, j, D]) - 1, inds[b, j]] = 1.0
    planted = np.zeros(0, np.int64)
    if plant:  # +-12 and +-30 on negatives, and one positive (gt == 1) at each sign
        values = np.array([12.0, -12.0, 30.0, -30.0, 12.0, -30.0], np.float32)
        ones = np.flatnonzero(heatmap.reshape(-1) == 1.0)
        others = np.flatnonzero(heatmap.reshape(-1) < 1.0)
        assert len(ones) >= 2
        planted = np.concatenate([rng.choice(others, 4, replace=False), rng.choice(ones, 2, replace=False)])
        hm.reshape(-1)[planted] = values
    code_weights = (0.5 + rng.random(D)).astype(np.float32)
    code_weights[3] = 0.2
    return dict(hm=hm, heatmap=heatmap, maps=maps, target_boxes=target, inds=inds, masks=mask, code_weights=code_weights,
                loc_weight=0.25, planted=planted)
