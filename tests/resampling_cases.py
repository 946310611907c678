"""Float64 numpy restatement of the resize unit (csrc/resize_line.h, csrc/resize.hip) and the case table its tests share.

The functions mirror the header line by line: `coord`, `causal_start`, `anticausal_start`, `fold`, `extend`, `weights3`, `taps`,
`label_vote`; `prefilter_line` and `resize_line` put them together for one line, `prefilter`, `resize`, `resize_labels` and
`resize_labels_axis` for a [NC, D, H, W] volume, as the kernels do.  tests/test_resampling_cases_cpu.py checks the restatement
against scipy.ndimage.zoom / map_coordinates themselves and against the header built as a host program; the GPU tests compare the
kernels with it."""
import numpy as np

POLE = np.sqrt(3.0) - 2.0


def coord(o, n_in, n_out):
    return (np.asarray(o, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5


def causal_start(x_first):
    return 6.0 * x_first / (1.0 - POLE)


def anticausal_start(cp_last, x_last):
    z = POLE
    s = 6.0 * x_last / (1.0 - z)
    return -(s * z / (1.0 - z) + (cp_last - s) * z / (1.0 - z * z))


def fold(m):
    """c[-m] = a c[0] + b c[1]"""
    z = POLE
    zm = z if m == 1 else z * z
    b = (1.0 - zm) / (5.0 + z)
    return (4.0 + z) * b + zm, b


def extend(c0, c1, m):
    a, b = fold(m)
    return a * c0 + b * c1


def weights3(t):
    u = 1.0 - t
    return [u * u * u / 6.0, (3.0 * t * t * t - 6.0 * t * t + 4.0) / 6.0, (3.0 * u * u * u - 6.0 * u * u + 4.0) / 6.0, t * t * t / 6.0]


def tap_base3(o, n_in, n_out):
    return int(np.floor(coord(o, n_in, n_out))) - 1


def ntaps(order, n_in, n_out):
    return 1 if n_in == n_out or order == 0 else 2 if order == 1 else 4


def taps(order, o, n_in, n_out):
    """-> (idx, w): out[o] = sum_k w[k] line[idx[k]]; every idx in [0, n_in)."""
    if n_in == n_out:
        return [o], [1.0]
    x = float(coord(o, n_in, n_out))
    if order == 0:
        return [min(max(int(np.floor(x + 0.5)), 0), n_in - 1)], [1.0]
    if order == 1:
        xc = min(max(x, 0.0), float(n_in - 1))
        i = int(np.floor(xc))
        t = xc - i
        return [i, min(i + 1, n_in - 1)], [1.0 - t, t]
    fl = np.floor(x)
    base = int(fl) - 1
    w = weights3(x - fl)
    if n_in == 1:
        return [0, 0, 0, 0], [w[0] + w[1] + w[2] + w[3], 0.0, 0.0, 0.0]
    a1, b1 = fold(1)
    a2, b2 = fold(2)
    if base == -2:
        w[2] += w[0] * a2 + w[1] * a1; w[3] += w[0] * b2 + w[1] * b1; w[0] = 0.0; w[1] = 0.0
    elif base == -1:
        w[1] += w[0] * a1; w[2] += w[0] * b1; w[0] = 0.0
    over = base + 3 - (n_in - 1)
    if over == 2:
        w[1] += w[2] * a1 + w[3] * a2; w[0] += w[2] * b1 + w[3] * b2; w[2] = 0.0; w[3] = 0.0
    elif over == 1:
        w[2] += w[3] * a1; w[1] += w[3] * b1; w[3] = 0.0
    return [min(max(base + k, 0), n_in - 1) for k in range(4)], w


def label_vote(lab, w, strict):
    res, found = 0.0, False
    for k in range(len(lab)):
        if w[k] < 0.0:
            continue
        s = sum(w[j] for j in range(len(lab)) if w[j] >= 0.0 and lab[j] == lab[k])
        if (s > 0.5 if strict else s >= 0.5) and (not found or lab[k] > res):
            res, found = lab[k], True
    return res


# ---- one line ----------------------------------------------------------------------------------------------------------------------
def prefilter_line(x, store=np.float64):
    """The coefficients of the line extended by its edge values; `store` is the type they are rounded to once (float32 on the device)."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    if n == 1:
        return x.astype(store).astype(np.float64)
    z = POLE
    cp = np.empty(n)
    cp[0] = causal_start(x[0])
    for k in range(1, n):
        cp[k] = 6.0 * x[k] + z * cp[k - 1]
    c = np.empty(n)
    c[n - 1] = anticausal_start(cp[n - 1], x[n - 1])
    for k in range(n - 2, -1, -1):
        c[k] = z * (c[k + 1] - cp[k])
    return c.astype(store).astype(np.float64)


def tap_matrix(order, n_in, n_out):
    """[n_out, n_in] float64: the resize of one axis as a matrix (rows hold the folded weights)."""
    m = np.zeros((n_out, n_in))
    for o in range(n_out):
        idx, w = taps(order, o, n_in, n_out)
        for i, wi in zip(idx, w):
            m[o, i] += wi
    return m


def resize_line(line, n_out, order, store=np.float64):
    line = np.asarray(line, dtype=np.float64)
    n = len(line)
    c = prefilter_line(line, store) if order == 3 and n != n_out else line
    return tap_matrix(order, n, n_out) @ c


# ---- volumes [NC, D, H, W] -----------------------------------------------------------------------------------------------------------
def prefilter(vol, axes, store=np.float32):
    """mt_resize_prefilter3: axes is the mask bit 0 W, bit 1 H, bit 2 D; passes in that order, rounded to `store` after each."""
    out = np.asarray(vol, dtype=np.float64).copy()
    for bit, ax in ((0, 3), (1, 2), (2, 1)):
        if axes >> bit & 1:
            x = np.moveaxis(out, ax, 0)                       # prefilter_line on every line at once: the recursion runs along axis 0
            n = x.shape[0]
            if n > 1:
                cp = np.empty_like(x)
                cp[0] = causal_start(x[0])
                for k in range(1, n):
                    cp[k] = 6.0 * x[k] + POLE * cp[k - 1]
                c = np.empty_like(x)
                c[n - 1] = anticausal_start(cp[n - 1], x[n - 1])
                for k in range(n - 2, -1, -1):
                    c[k] = POLE * (c[k + 1] - cp[k])
                x = c
            out = np.moveaxis(x.astype(store).astype(np.float64), 0, ax)
    return out


def resize(vol, out_shape, orders):
    """mt_resize on a volume that is already prefiltered where it has to be: float64 result (the device rounds it to float32)."""
    out = np.asarray(vol, dtype=np.float64)
    for ax in range(3):
        m = tap_matrix(orders[ax], out.shape[1 + ax], out_shape[ax])
        out = np.moveaxis(np.tensordot(m, out, axes=([1], [1 + ax])), 0, 1 + ax)
    return out


def resize_data(vol, out_shape, orders, store=np.float32):
    """Prefilter (the axes of order 3 that change) and resize: what one stage of resample_data_or_seg is on the device."""
    axes = sum(1 << (2 - ax) for ax in range(3) if orders[ax] == 3 and vol.shape[1 + ax] != out_shape[ax])
    return resize(prefilter(vol, axes, store) if axes else vol, out_shape, orders)


def resize_labels(seg, out_shape, strict=False):
    seg = np.asarray(seg, dtype=np.float64)
    NC, shape = seg.shape[0], seg.shape[1:]
    tp = [[taps(1, o, shape[ax], out_shape[ax]) for o in range(out_shape[ax])] for ax in range(3)]
    out = np.zeros((NC,) + tuple(out_shape))
    for od in range(out_shape[0]):
        idd, wd = tp[0][od]
        for oh in range(out_shape[1]):
            ih, wh = tp[1][oh]
            for ow in range(out_shape[2]):
                iw, ww = tp[2][ow]
                w = [a * b * c for a in wd for b in wh for c in ww]
                for nc in range(NC):
                    lab = [seg[nc, i, j, k] for i in idd for j in ih for k in iw]
                    out[nc, od, oh, ow] = label_vote(lab, w, strict)
    return out


def resize_labels_axis(seg, axis, out_n):
    shape = list(seg.shape[1:])
    shape[axis] = out_n
    return resize_labels(seg, shape, strict=True)


# ---- the case table ------------------------------------------------------------------------------------------------------------------
# (n_in, n_out) of one line: lengths 1, 2, 3, 4, 5, 33; up-sampling by more than 4x (coordinates reach -0.5 + eps); down-sampling by more
# than 2x; in == out.  Together every first tap -2 .. n - 2, i.e. every tap index -2 .. n + 1, occurs (asserted by the CPU test).
LINE_CASES = [(1, 1), (1, 5), (1, 40), (2, 2), (2, 9), (2, 64), (2, 1), (3, 3), (3, 14), (3, 1), (4, 4), (4, 17), (4, 7), (4, 1), (5, 5), (5, 23), (5, 2),
              (5, 7), (33, 33), (33, 140), (33, 13), (33, 47), (33, 16)]
ORDERS = (0, 1, 3)


def hu_line(n, seed):
    """HU-like values of range about 800."""
    rs = np.random.RandomState(seed)
    return (rs.rand(n) * 800.0 - 500.0).astype(np.float32)


def hu_volume(shape, seed, nc=1):
    """The generator of tests/test_preprocess_gpu.py's volumes in spirit: smooth structure times 600 plus 50."""
    from scipy import ndimage
    rs = np.random.RandomState(seed)
    return np.stack([ndimage.gaussian_filter(rs.randn(*shape), 1.0) * 600 + 50 for _ in range(nc)]).astype(np.float32)


def blocky_labels(shape, seed, nc=1):
    """Label maps with -1 in a margin, 0 background and boxes of 1..5."""
    rs = np.random.RandomState(seed)
    seg = np.zeros((nc,) + tuple(shape), dtype=np.float32)
    for c in range(nc):
        for lab in (1, 2, 3, 4, 5):
            for _ in range(2):
                lo = [rs.randint(0, max(1, n - 2)) for n in shape]
                sz = [rs.randint(1, max(2, n // 2)) for n in shape]
                seg[c, lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = lab
        if shape[1] > 4:
            seg[c, :, :2, :] = -1
        if shape[2] > 4:
            seg[c, :, :, -2:] = -1
    return seg


# kernel cases: (id, in shape, out shape, orders per axis D, H, W)
VOLUME_CASES = [
    ('iso_up_333', (5, 12, 12), (10, 24, 24), (3, 3, 3)),
    ('iso_down_333', (24, 26, 22), (13, 15, 14), (3, 3, 3)),
    ('iso_up_111', (9, 20, 18), (13, 27, 25), (1, 1, 1)),
    ('iso_000', (7, 24, 22), (14, 18, 17), (0, 0, 0)),
    ('slice_axis0_33', (9, 20, 18), (9, 27, 25), (0, 3, 3)),
    ('slice_axis1_33', (20, 9, 18), (27, 9, 25), (3, 0, 3)),
    ('slice_axis2_33', (20, 18, 9), (27, 25, 9), (3, 3, 0)),
    ('slice_axis0_11', (7, 24, 22), (7, 18, 17), (1, 1, 1)),
    ('z_axis0_3', (9, 27, 25), (13, 27, 25), (3, 0, 0)),
    ('z_axis1_1', (27, 9, 25), (27, 13, 25), (0, 1, 0)),
    ('z_axis2_3', (14, 18, 7), (14, 18, 17), (1, 1, 3)),
    ('z_axis0_0', (7, 18, 17), (14, 18, 17), (0, 3, 1)),
    ('short_lines', (1, 2, 3), (4, 7, 9), (3, 3, 3)),
    ('mixed_310', (4, 5, 33), (9, 3, 70), (3, 1, 0)),
    ('large', (40, 70, 130), (55, 50, 200), (3, 3, 3)),
]
