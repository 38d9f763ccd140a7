"""numpy float64 statement of CenterHead's loss for one head (TEST INFRASTRUCTURE ONLY): what csrc/center_loss.hip computes,
forward values and every gradient, evaluated on the float32 inputs.

    p        = clamp(sigmoid(x), f32(1e-4), f32(1 - 1e-4))        (the bounds float32 sees, not the double constants)
    pos      = sum_{gt == 1} log(p) (1 - p)^2,   neg = sum_{gt < 1} log(1 - p) p^2 (1 - gt)^4,   num_pos = #{gt == 1}
    hm_loss  = -(pos + neg) / num_pos if num_pos > 0 else -neg
    num      = #{mask != 0};   per_dim[d] = sum_{b,j unmasked, 0 <= ind < H W} |map_d[b, :, ind] - target[b, j, d]| / max(num, 1)
    loc_loss = loc_weight sum_d code_weights[d] per_dim[d]

A masked-out slot is never read (NaN targets, an index of 2^40); an unmasked slot whose index lies outside the map counts
in ``num`` and contributes nothing.  Gradients: through the clamp as torch does (zero where the sigmoid lies outside the
bounds); the regression gradient of a cell is the sum of its slots in ascending j, sign(0) = 0."""
import numpy as np

LO = np.float32(1e-4)
HI = np.float32(1 - 1e-4)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _prob(hm):
    """clamped p, 1 - p (the small one never formed by cancellation), and where the gradient passes the clamp"""
    x = np.asarray(hm, dtype=np.float64)
    s, t = _sigmoid(x), _sigmoid(-x)
    lo, hi = np.float64(LO), np.float64(HI)
    inside = (s >= lo) & (s <= hi)
    p = np.clip(s, lo, hi)
    q = np.where(s < lo, 1.0 - lo, np.where(s > hi, 1.0 - hi, t))
    return p, q, inside


def _slots(maps, inds, masks):
    B, HW = maps[0].shape[0], maps[0].shape[2] * maps[0].shape[3]
    unmasked = np.asarray(masks) != 0
    ind = np.where(unmasked, np.asarray(inds), -1)  # a masked-out slot's index is not read
    valid = unmasked & (ind >= 0) & (ind < HW)
    return B, HW, unmasked, np.where(valid, ind, 0), valid


def forward(hm, heatmap, maps, target_boxes, inds, masks, code_weights, loc_weight):
    """dict(hm_loss, loc_loss, per_dim (D), num_pos, num) in float64 / int"""
    p, q, _ = _prob(hm)
    gt = np.asarray(heatmap, dtype=np.float64)
    is_pos, is_neg = gt == 1, gt < 1
    pos = float((np.log(p) * q * q)[is_pos].sum())
    neg = float((np.log(q) * p * p * (1.0 - gt) ** 4)[is_neg].sum())
    num_pos = int(is_pos.sum())
    hm_loss = -(pos + neg) / num_pos if num_pos > 0 else -neg
    B, HW, unmasked, ind, valid = _slots(maps, inds, masks)
    num = int(unmasked.sum())
    per_dim, d0 = [], 0
    for m in maps:
        flat = np.asarray(m, dtype=np.float64).reshape(B, m.shape[1], HW)
        for c in range(m.shape[1]):
            pred = np.take_along_axis(flat[:, c], ind, axis=1)
            tgt = np.where(valid, np.asarray(target_boxes)[:, :, d0 + c], 0.0).astype(np.float64)
            per_dim.append(float(np.abs(pred - tgt)[valid].sum()) / max(num, 1))
        d0 += m.shape[1]
    per_dim = np.array(per_dim, dtype=np.float64)
    loc_loss = float(loc_weight) * float((np.asarray(code_weights, dtype=np.float64) * per_dim).sum())
    return dict(hm_loss=hm_loss, loc_loss=loc_loss, per_dim=per_dim, num_pos=num_pos, num=num)


def backward(hm, heatmap, maps, target_boxes, inds, masks, code_weights, loc_weight, g_hm=1.0, g_loc=1.0):
    """(d_hm, [d_map_k]) of g_hm hm_loss + g_loc loc_loss in float64"""
    p, q, inside = _prob(hm)
    gt = np.asarray(heatmap, dtype=np.float64)
    is_pos, is_neg = gt == 1, gt < 1
    num_pos = int(is_pos.sum())
    # (d/dp of the term) s (1 - s); inside the clamp s = p
    t = np.where(is_pos, q ** 3 - 2.0 * q * q * p * np.log(p),
                 np.where(is_neg, (2.0 * p * p * q * np.log(q) - p ** 3) * (1.0 - gt) ** 4, 0.0))
    d_hm = np.where(inside, -(float(g_hm) / max(num_pos, 1)) * t, 0.0)
    B, HW, unmasked, ind, valid = _slots(maps, inds, masks)
    num = int(unmasked.sum())
    d_maps, d0 = [], 0
    cw = np.asarray(code_weights, dtype=np.float64)
    bs, js = np.nonzero(valid)  # row-major: ascending j inside a sample
    for m in maps:
        g = np.zeros((B, m.shape[1], HW), dtype=np.float64)
        flat = np.asarray(m, dtype=np.float64).reshape(B, m.shape[1], HW)
        for c in range(m.shape[1]):
            cells = ind[bs, js]
            diff = flat[bs, c, cells] - np.asarray(target_boxes)[bs, js, d0 + c].astype(np.float64)
            np.add.at(g[:, c], (bs, cells), float(g_loc) * float(loc_weight) * cw[d0 + c] * np.sign(diff) / max(num, 1))
        d0 += m.shape[1]
        d_maps.append(g.reshape(m.shape))
    return d_hm, d_maps
