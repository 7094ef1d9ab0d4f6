"""numpy restatement of include/rfd.h, "frames in camera and decoder formats": the layouts, the unfiltered chroma replication, the
four fixed-point tables and the byte moves.  Everything is int32 as in the header; numpy's >> on a signed array is arithmetic.

A frame here is (format, width, height, planes[, color]): planes the 2-D u8 arrays of rfd_frame_layout_of, [rows, row_bytes]."""
import numpy as np

BGR, RGB, BGRA, RGBA, GRAY, NV12, NV21, I420, YUYV, UYVY = range(10)
NAMES = ("bgr", "rgb", "bgra", "rgba", "gray", "nv12", "nv21", "i420", "yuyv", "uyvy")
BT601_LIMITED, BT601_FULL, BT709_LIMITED, BT709_FULL = range(4)

# colour: CY, CVR, CUG, CVG, CUB, limited
TABLE = {
    BT601_LIMITED: (1220542, 1673527, -409993, -852492, 2116026, True),
    BT601_FULL: (1048576, 1470104, -360853, -748826, 1858077, False),
    BT709_LIMITED: (1220542, 1880097, -223347, -558891, 2214593, True),
    BT709_FULL: (1048576, 1651297, -196423, -490864, 1945738, False),
}
# the real coefficients the tables round: CY, CVR, CUG, CVG, CUB
REAL = {
    BT601_LIMITED: (1.164, 1.596, -0.391, -0.813, 2.018),
    BT601_FULL: (1.0, 1.402, -0.344136, -0.714136, 1.772),
    BT709_LIMITED: (1.164, 1.793, -0.213, -0.533, 2.112),
    BT709_FULL: (1.0, 1.5748, -0.187324, -0.468124, 1.8556),
}


def layout(fmt, w, h):
    """-> [(row_bytes, rows)] per plane"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt in (BGR, RGB):
        return [(3 * w, h)]
    if fmt in (BGRA, RGBA):
        return [(4 * w, h)]
    if fmt == GRAY:
        return [(w, h)]
    if fmt in (NV12, NV21):
        return [(w, h), (2 * cw, ch)]
    if fmt == I420:
        return [(w, h), (cw, ch), (cw, ch)]
    if fmt in (YUYV, UYVY):
        return [(4 * cw, h)]
    raise ValueError(fmt)


def shifted(Y, U, V, color):
    """arrays of equal shape (any integer type, values 0 .. 255) -> [..., 3] i32: the B, G, R sums after >> 20, before the clamp"""
    cy, cvr, cug, cvg, cub, limited = TABLE[color]
    y = np.asarray(Y).astype(np.int32)
    u = np.asarray(U).astype(np.int32) - 128
    v = np.asarray(V).astype(np.int32) - 128
    if limited:
        y = np.maximum(y - 16, 0)
    ys = np.int32(cy) * y
    r = (ys + np.int32(cvr) * v + np.int32(524288)) >> 20
    g = (ys + np.int32(cug) * u + np.int32(cvg) * v + np.int32(524288)) >> 20
    b = (ys + np.int32(cub) * u + np.int32(524288)) >> 20
    assert r.dtype == np.int32 and g.dtype == np.int32 and b.dtype == np.int32
    return np.stack([b, g, r], -1)


def yuv_to_bgr(Y, U, V, color):
    """-> [..., 3] u8, B G R"""
    return np.clip(shifted(Y, U, V, color), 0, 255).astype(np.uint8)


def _up(c, w, h, fx, fy):
    """every sample of a chroma plane under the fx x fy luma samples it serves, cropped to w x h"""
    return np.repeat(np.repeat(c, fy, 0), fx, 1)[:h, :w]


def convert(fmt, w, h, planes, color=BT601_LIMITED):
    """-> [h, w, 3] u8 BGR"""
    for a, (rb, rows) in zip(planes, layout(fmt, w, h)):
        assert a.dtype == np.uint8 and a.shape == (rows, rb), (NAMES[fmt], a.shape, (rows, rb))
    p = planes[0]
    if fmt == BGR:
        return p.reshape(h, w, 3).copy()
    if fmt == RGB:
        return p.reshape(h, w, 3)[:, :, ::-1].copy()
    if fmt == BGRA:
        return p.reshape(h, w, 4)[:, :, :3].copy()
    if fmt == RGBA:
        return p.reshape(h, w, 4)[:, :, 2::-1].copy()
    if fmt == GRAY:
        return np.repeat(p[:, :, None], 3, 2)
    if fmt in (NV12, NV21):
        c = planes[1].reshape(planes[1].shape[0], -1, 2)
        u, v = (c[:, :, 0], c[:, :, 1]) if fmt == NV12 else (c[:, :, 1], c[:, :, 0])
        return yuv_to_bgr(p, _up(u, w, h, 2, 2), _up(v, w, h, 2, 2), color)
    if fmt == I420:
        return yuv_to_bgr(p, _up(planes[1], w, h, 2, 2), _up(planes[2], w, h, 2, 2), color)
    q = p.reshape(h, -1, 4)                                      # one pixel pair per 4 bytes
    yb = 0 if fmt == YUYV else 1
    y = q[:, :, [yb, yb + 2]].reshape(h, -1)[:, :w]
    return yuv_to_bgr(y, _up(q[:, :, 1 - yb], w, h, 2, 1), _up(q[:, :, 3 - yb], w, h, 2, 1), color)


def convert_frame(frame):
    return convert(frame[0], frame[1], frame[2], frame[3], frame[4] if len(frame) > 4 else BT601_LIMITED)


# ---- one image in several layouts: what the layout-agreement tests and the sweeps build their planes from ----
def planes_420(fmt, y, u, v):
    """y [h, w], u and v [ch, cw] -> the planes of NV12, NV21 or I420"""
    if fmt == I420:
        return [y.copy(), u.copy(), v.copy()]
    a, b = (u, v) if fmt == NV12 else (v, u)
    return [y.copy(), np.stack([a, b], -1).reshape(u.shape[0], -1)]


def planes_422(fmt, y, u, v):
    """y [h, w], u and v [h, cw] -> the plane of YUYV or UYVY; the unused luma byte of an odd row's last pair is 0"""
    h, w = y.shape
    cw = (w + 1) // 2
    yy = np.zeros((h, 2 * cw), np.uint8)
    yy[:, :w] = y
    parts = [yy[:, 0::2], u, yy[:, 1::2], v] if fmt == YUYV else [u, yy[:, 0::2], v, yy[:, 1::2]]
    return [np.stack(parts, -1).reshape(h, 4 * cw)]


def random_planes(rng, fmt, w, h):
    return [rng.integers(0, 256, (rows, rb), dtype=np.uint8) for rb, rows in layout(fmt, w, h)]
