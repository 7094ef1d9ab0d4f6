"""Constructed inputs of the frame conversion (include/rfd.h, "frames in camera and decoder formats") with the answer WRITTEN
DOWN from the arithmetic of the header, worked by hand with exact integers -- not computed by tests/frame_ref.py, which is held
to these values (tests/test_frame_cpu.py), as are all three forms of the library (tests/test_frame_gpu.py).

YUV[colour] lists (name, (Y, U, V), (B, G, R)).  With u = U - 128, v = V - 128, y = Y - 16 clamped at 0 (limited) or Y (full):
e.g. BT601_LIMITED "mid" (120, 90, 200): y = 104, u = -38, v = 72; CY y = 126936368;
  B = (126936368 - 38 * 2116026 + 524288) >> 20 = 47051668 >> 20 = 44
  G = (126936368 + 38 * 409993 - 72 * 852492 + 524288) >> 20 = 81660966 >> 20 = 77
  R = (126936368 + 72 * 1673527 + 524288) >> 20 = 247954600 >> 20 = 236."""
import numpy as np

import frame_ref as FR

YUV = {
    FR.BT601_LIMITED: [
        ("black", (16, 128, 128), (0, 0, 0)),             # 524288 >> 20 = 0
        ("white", (235, 128, 128), (255, 255, 255)),      # 219 * 1220542 + 524288 = 267822986 >> 20 = 255
        ("grey", (126, 128, 128), (128, 128, 128)),       # 110 * 1220542 + 524288 = 134783908 >> 20 = 128
        ("below_16", (5, 128, 128), (0, 0, 0)),           # y = max(5 - 16, 0) = 0: as black
        ("above_235", (255, 128, 128), (255, 255, 255)),  # 292233826 >> 20 = 278, clamped
        ("r_high", (235, 128, 255), (255, 152, 255)),     # R 480360915 >> 20 = 458; G 159556502 >> 20 = 152
        ("r_low", (16, 128, 0), (0, 104, 0)),             # R -213687168 >> 20 = -204; G 109643264 >> 20 = 104
        ("b_high", (235, 255, 128), (255, 205, 255)),     # B 536558288 >> 20 = 511 (the largest sum); G 215753875 >> 20 = 205
        ("b_low", (16, 0, 128), (0, 50, 0)),              # B -270327040 >> 20 = -258; G 53003392 >> 20 = 50
        ("g_high", (235, 0, 0), (0, 255, 51)),            # G 429421066 >> 20 = 409; B -3028342 >> 20 = -3; R 53611530 >> 20 = 51
        ("g_low", (16, 255, 255), (255, 0, 203)),         # G -159811307 >> 20 = -153; B 269259590 >> 20 = 256; R 213062217 >> 20 = 203
        ("mid", (120, 90, 200), (44, 77, 236)),
    ],
    FR.BT601_FULL: [
        ("black", (0, 128, 128), (0, 0, 0)),
        ("white", (255, 128, 128), (255, 255, 255)),      # 255 * 1048576 + 524288 = 267911168 >> 20 = 255
        ("y_unchanged", (77, 128, 128), (77, 77, 77)),    # (77 << 20) + 524288 >> 20 = 77: every Y passes through at u = v = 0
        ("r_high", (255, 128, 255), (255, 164, 255)),     # R 454614376 >> 20 = 433; G 172810266 >> 20 = 164
        ("r_low", (0, 128, 0), (0, 91, 0)),               # R -187649024 >> 20 = -179; G 96374016 >> 20 = 91
        ("b_high", (255, 255, 128), (255, 211, 255)),     # B 503886947 >> 20 = 480; G 222082837 >> 20 = 211
        ("b_low", (0, 0, 128), (0, 44, 0)),               # B -237309568 >> 20 = -227; G 46713472 >> 20 = 44
        ("g_high", (255, 0, 0), (28, 255, 76)),           # G 409950080 >> 20 = 390; B 30077312 >> 20 = 28; R 79737856 >> 20 = 76
        ("g_low", (0, 255, 255), (225, 0, 178)),          # G -140404945 >> 20 = -134; B 236500067 >> 20 = 225; R 187227496 >> 20 = 178
        ("mid", (120, 90, 200), (53, 82, 221)),           # B 55746482, G 86150350, R 232200896
    ],
    FR.BT709_LIMITED: [
        ("black", (16, 128, 128), (0, 0, 0)),
        ("white", (235, 128, 128), (255, 255, 255)),
        ("grey", (126, 128, 128), (128, 128, 128)),
        ("below_16", (5, 128, 128), (0, 0, 0)),
        ("above_235", (255, 128, 128), (255, 255, 255)),
        ("r_high", (235, 128, 255), (255, 187, 255)),     # R 506595305 >> 20 = 483; G 196843829 >> 20 = 187
        ("r_low", (16, 128, 0), (0, 68, 0)),              # R -240128128 >> 20 = -230; G 72062336 >> 20 = 68
        ("b_high", (235, 255, 128), (255, 228, 255)),     # B 549076297 >> 20 = 523; G 239457917 >> 20 = 228
        ("b_low", (16, 0, 128), (0, 27, 0)),              # B -282943616 >> 20 = -270; G 29112704 >> 20 = 27
        ("g_high", (235, 0, 0), (0, 255, 25)),            # G 367949450 >> 20 = 350; B -15644918 >> 20 = -15; R 27170570 >> 20 = 25
        ("g_low", (16, 255, 255), (255, 0, 228)),         # G -98819938 >> 20 = -95; B 281777599 >> 20 = 268; R 239296607 >> 20 = 228
        ("mid", (120, 90, 200), (41, 91, 250)),           # B 43306122, G 95707690, R 262827640
    ],
    FR.BT709_FULL: [
        ("black", (0, 128, 128), (0, 0, 0)),
        ("white", (255, 128, 128), (255, 255, 255)),
        ("y_unchanged", (77, 128, 128), (77, 77, 77)),
        ("r_high", (255, 128, 255), (255, 196, 255)),     # R 477625887 >> 20 = 455; G 205571440 >> 20 = 196
        ("r_low", (0, 128, 0), (0, 60, 0)),               # R -210841728 >> 20 = -202; G 63354880 >> 20 = 60
        ("b_high", (255, 255, 128), (255, 231, 255)),     # B 515019894 >> 20 = 491; G 242965447 >> 20 = 231
        ("b_low", (0, 0, 128), (0, 24, 0)),               # B -248530176 >> 20 = -238; G 25666432 >> 20 = 24
        ("g_high", (255, 0, 0), (17, 255, 53)),           # G 355883904 >> 20 = 339; B 18856704 >> 20 = 17; R 56545152 >> 20 = 53
        ("g_low", (0, 255, 255), (236, 0, 200)),          # G -86761161 >> 20 = -83; B 247633014 >> 20 = 236; R 210239007 >> 20 = 200
        ("mid", (120, 90, 200), (49, 93, 233)),           # B 52415364, G 98475274, R 245246792
    ],
}

# >> 20 of a NEGATIVE sum is a floor, not a truncation toward zero: colour, (Y, U, V), the B sum, its >> 20.  In all four the
# luma term is 0 and u = -1, so the B sum is 524288 - CUB, between -2 * 2^20 and -2^20: the floor is -2, a truncation gives -1.
# (After the clamp both are 0: the pixel cannot tell them apart, the sum can.)
FLOOR = [
    (FR.BT601_LIMITED, (16, 127, 128), -1591738, -2),
    (FR.BT601_FULL, (0, 127, 128), -1333789, -2),
    (FR.BT709_LIMITED, (16, 127, 128), -1690305, -2),
    (FR.BT709_FULL, (0, 127, 128), -1421450, -2),
]

# The byte formats: a 3 x 2 image given pixel by pixel as (B, G, R), and an alpha per pixel that no output may depend on
# (0 and 255 among them).
BYTE_PIXELS = [[(1, 2, 3), (250, 128, 7), (0, 255, 0)], [(90, 80, 70), (255, 0, 255), (13, 17, 19)]]
BYTE_ALPHA = [[0, 255, 128], [255, 0, 1]]
GRAY_PIXELS = [[0, 255, 16], [235, 128, 77]]     # B = G = R = Y, no range expansion: 16 stays 16


def yuv_image(color):
    """-> (y [2, 2k], u [1, k], v [1, k], want [2, 2k, 3]): case j of YUV[color] fills the 2 x 2 block at column 2 j, so that the
    4:2:0 formats (one chroma sample per block) and the 4:2:2 formats (one per row of it) hold the same image"""
    cases = YUV[color]
    k = len(cases)
    y, u, v, want = np.zeros((2, 2 * k), np.uint8), np.zeros((1, k), np.uint8), np.zeros((1, k), np.uint8), np.zeros((2, 2 * k, 3), np.uint8)
    for j, (_, (Y, U, V), bgr) in enumerate(cases):
        y[:, 2 * j:2 * j + 2], u[0, j], v[0, j] = Y, U, V
        want[:, 2 * j:2 * j + 2] = bgr
    return y, u, v, want


def frames():
    """every constructed case as (name, frame, want): frame = (format, width, height, planes, color), want [h, w, 3] u8 BGR"""
    out = []
    for color in sorted(YUV):
        y, u, v, want = yuv_image(color)
        h, w = y.shape
        for fmt in (FR.NV12, FR.NV21, FR.I420):
            out.append(("%s_colour%d" % (FR.NAMES[fmt], color), (fmt, w, h, FR.planes_420(fmt, y, u, v), color), want))
        for fmt in (FR.YUYV, FR.UYVY):
            out.append(("%s_colour%d" % (FR.NAMES[fmt], color), (fmt, w, h, FR.planes_422(fmt, y, np.repeat(u, 2, 0), np.repeat(v, 2, 0)), color), want))
    bgr = np.array(BYTE_PIXELS, np.uint8)
    a = np.array(BYTE_ALPHA, np.uint8)[:, :, None]
    h, w = bgr.shape[:2]
    rgb = bgr[:, :, ::-1]
    out.append(("bgr", (FR.BGR, w, h, [bgr.reshape(h, 3 * w).copy()], 0), bgr))
    out.append(("rgb", (FR.RGB, w, h, [rgb.reshape(h, 3 * w).copy()], 0), bgr))
    for name, alpha in (("alpha", a), ("alpha_0", a * 0), ("alpha_255", a * 0 + 255)):
        out.append(("bgra_" + name, (FR.BGRA, w, h, [np.concatenate([bgr, alpha], 2).reshape(h, 4 * w)], 0), bgr))
        out.append(("rgba_" + name, (FR.RGBA, w, h, [np.concatenate([rgb, alpha], 2).reshape(h, 4 * w)], 0), bgr))
    g = np.array(GRAY_PIXELS, np.uint8)
    out.append(("gray", (FR.GRAY, g.shape[1], g.shape[0], [g.copy()], 0), np.repeat(g[:, :, None], 3, 2)))
    return out
