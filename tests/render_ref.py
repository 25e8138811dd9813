"""numpy restatement of csrc/render.hip (include/mvx_hip.h "Frame rendering"): float64 geometry, Python integers wherever a
pixel is decided, one pixel at a time.  No torch, no library.  The library is built with -ffp-contract=off, so every f64
expression below is written with the same operations in the same order; cos and sin are the only calls whose last bit may
differ between the two sides (the GPU tests keep every endpoint 1e-6 px away from a pixel boundary)."""
import math

import numpy as np

BAD_BOX = 1
COORD_LIMIT = float(1 << 24)
# corners of Calc.bbox3d2corner: 0..3 the top face, 4..7 the bottom face, BEV corner k & 3 = (+,+), (-,+), (-,-), (+,-)
CAMERA_SEGMENTS = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7), (0, 7), (3, 4))


def segment_pixels(r0, c0, r1, c1):
    """Every pixel (row, col) of the segment, k = 0..n, unclipped: one Python int expression each."""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    rows_major = abs(r1 - r0) >= abs(c1 - c0)
    a, b = ((r0, c0), (r1, c1)) if rows_major else ((c0, r0), (c1, r1))
    if b < a:                                       # the end with the smaller (major, minor) pair first
        a, b = b, a
    n, dq = b[0] - a[0], b[1] - a[1]
    sgn = -1 if dq < 0 else 1
    out = []
    for k in range(n + 1):
        major = a[0] + k
        minor = a[1] if n == 0 else a[1] + sgn * ((2 * k * abs(dq) + n) // (2 * n))
        out.append((major, minor) if rows_major else (minor, major))
    return out


def clipped_k_range(r0, c0, r1, c1, H, W):
    """(first k, last k, rows_major, first end, n, dq) of the k whose MAJOR coordinate is inside the image."""
    rows_major = abs(r1 - r0) >= abs(c1 - c0)
    a, b = ((r0, c0), (r1, c1)) if rows_major else ((c0, r0), (c1, r1))
    if b < a:
        a, b = b, a
    n = b[0] - a[0]
    M = H if rows_major else W
    return max(0, -a[0]), min(n, M - 1 - a[0]), rows_major, a, n, b[1] - a[1]


def draw_segment(plane, r0, c0, r1, c1, T, word):
    """max(word) into plane (H, W) along the segment; only the k inside the image are visited (a segment that leaves the
    image by 10^5 pixels costs at most max(H, W) steps here too)."""
    H, W = plane.shape
    klo, khi, rows_major, a, n, dq = clipped_k_range(int(r0), int(c0), int(r1), int(c1), H, W)
    sgn = -1 if dq < 0 else 1
    for k in range(klo, khi + 1):
        major = a[0] + k
        minor = a[1] if n == 0 else a[1] + sgn * ((2 * k * abs(dq) + n) // (2 * n))
        r, c = (major, minor) if rows_major else (minor, major)
        if not (0 <= r < H and 0 <= c < W):
            continue
        for dr in range(-(T // 2), T - 1 - (T // 2) + 1):
            for dc in range(-(T // 2), T - 1 - (T // 2) + 1):
                rr, cc = r + dr, c + dc
                if 0 <= rr < H and 0 <= cc < W and word > plane[rr, cc]:
                    plane[rr, cc] = word


def clampq(v, hi):
    if not v > 0.0:
        return 0
    if v >= float(hi):
        return hi
    return int(math.floor(v))


def bev_corner(b, k, c, s):
    px = (0.5 if k in (0, 3) else -0.5) * b[3]
    py = (0.5 if k < 2 else -0.5) * b[4]
    return (px * c + py * s) + b[0], (-px * s + py * c) + b[1]


def _box64(box):
    b = [float(np.float64(np.float32(v))) for v in box]
    return b, all(math.isfinite(v) for v in b)


def bev_endpoints(box, x0, y0, res):
    """The 5 segments of a finite box as ((i0, j0), (i1, j1)) PRE-FLOOR cell coordinates (x - x0) / res, (y - y0) / res."""
    b, _ = _box64(box)
    c, s = math.cos(b[6]), math.sin(b[6])
    xy = [bev_corner(b, k, c, s) for k in range(4)]
    px = 0.5 * b[3]
    segs = [(xy[k], xy[(k + 1) & 3]) for k in range(4)] + [((b[0], b[1]), (px * c + b[0], -px * s + b[1]))]
    return [tuple(((X - x0) / res, (Y - y0) / res) for X, Y in sg) for sg in segs]


def camera_endpoints(box, mat, z_near):
    """The segments of a finite box that survive the clip, as ((row0, col0), (row1, col1)) PRE-FLOOR pixel coordinates."""
    b, _ = _box64(box)
    c, s = math.cos(b[6]), math.sin(b[6])
    m = [float(v) for v in np.asarray(mat, dtype=np.float64).reshape(16)]
    hom = []
    for k in range(8):
        X, Y = bev_corner(b, k & 3, c, s)
        Z = b[2] + b[5] if k < 4 else b[2]
        hom.append([((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z) + m[4 * r + 3] for r in range(3)])
    out = []
    for ka, kb in CAMERA_SEGMENTS:
        e = [list(hom[ka]), list(hom[kb])]
        behind = [e[0][2] < z_near, e[1][2] < z_near]
        if behind[0] and behind[1]:
            continue
        if behind[0] != behind[1]:
            i = 0 if behind[0] else 1
            g = 1 - i
            t = (z_near - e[i][2]) / (e[g][2] - e[i][2])
            e[i] = [e[i][0] + t * (e[g][0] - e[i][0]), e[i][1] + t * (e[g][1] - e[i][1]), z_near]
        with np.errstate(all='ignore'):
            out.append(tuple((float(np.float64(p[1]) / np.float64(p[2])), float(np.float64(p[0]) / np.float64(p[2]))) for p in e))
    return out


def _pixel_ok(r, c):
    return abs(r) < COORD_LIMIT and abs(c) < COORD_LIMIT         # a NaN fails


def _draw_boxes(overlay, status, f, boxes, n_boxes, colors, T, segments_of):
    """segments_of(box) -> [((row0, col0), (row1, col1))] in floored float64 pixel coordinates; one bad end drops the box."""
    B = boxes.shape[1]
    for bi in range(min(max(int(n_boxes[f]), 0), B)):
        word = int(colors[f, bi]) & 0xFFFFFFFF
        if word == 0:
            continue
        _, finite = _box64(boxes[f, bi])
        segs = segments_of(boxes[f, bi]) if finite else None
        if segs is None or not all(_pixel_ok(*p) and _pixel_ok(*q) for p, q in segs):
            status[f] |= BAD_BOX
            continue
        for p, q in segs:
            draw_segment(overlay[f], int(p[0]), int(p[1]), int(q[0]), int(q[1]), T, word)


def _rgb(word):
    return ((word >> 16) & 255, (word >> 8) & 255, word & 255)


def render_bev(points6, n_points, boxes, n_boxes, colors, x0, y0, res, z0, z1, H, W, lut, color_by, cmax, background, T):
    """(image u8 (F, H, W, 3), status i32 (F,)).  points6 (F, cap, >= 6) f32, colors (F, B) int (the u32 words, any sign)."""
    F, cap = points6.shape[:2]
    key = np.zeros((F, H, W), np.int64)
    cnt = np.zeros((F, H, W), np.int64)
    overlay = np.zeros((F, H, W), np.int64)
    status = np.zeros((F,), np.int32)
    x0, y0, res, z0, zspan = float(x0), float(y0), float(res), float(z0), float(z1) - float(z0)
    for f in range(F):
        for p in range(min(max(int(n_points[f]), 0), cap)):
            x, y, z, r = (float(np.float64(v)) for v in points6[f, p, :4])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                continue
            di, dj = math.floor((x - x0) / res), math.floor((y - y0) / res)
            if not (0 <= di < H and 0 <= dj < W):
                continue
            zq = clampq((z - z0) / zspan * 65535.0, 65535)
            iq = clampq(r * 255.0, 255) if not math.isnan(r) else 0
            at = (f, H - 1 - di, W - 1 - dj)
            key[at] = max(key[at], ((zq << 8) | iq) + 1)
            cnt[at] += 1

    def segments_of(box):
        out = []
        for p, q in bev_endpoints(box, x0, y0, res):
            out.append(tuple((float(H - 1) - math.floor(e[0]) if math.isfinite(e[0]) else math.nan,
                              float(W - 1) - math.floor(e[1]) if math.isfinite(e[1]) else math.nan) for e in (p, q)))
        return out

    if boxes is not None:
        for f in range(F):
            _draw_boxes(overlay, status, f, boxes, n_boxes, colors, T, segments_of)
    img = np.zeros((F, H, W, 3), np.uint8)
    lut = np.asarray(lut).astype(np.int64)
    for f in range(F):
        for r in range(H):
            for c in range(W):
                if overlay[f, r, c]:
                    img[f, r, c] = _rgb(int(overlay[f, r, c]))
                elif key[f, r, c] == 0:
                    img[f, r, c] = _rgb(int(background))
                else:
                    kq = int(key[f, r, c]) - 1
                    idx = (kq & 255) if color_by == 'intensity' else (kq >> 16)
                    shade = 64 + 191 * min(int(cnt[f, r, c]), cmax) // cmax
                    img[f, r, c] = [int(lut[idx, ch]) * shade // 255 for ch in range(3)]
    return img, status


def render_camera(points6, n_points, boxes, n_boxes, colors, mats, z_near, depth_max, H, W, lut, R, images, bgr, T):
    """(image u8 (F, H, W, 3), status i32 (F,)).  mats f64 (F, 4, 4); images u8 (F, H, W, 3) or None."""
    F, cap = points6.shape[:2]
    EMPTY = 0xFFFFFFFF
    depth = np.full((F, H, W), EMPTY, np.int64)
    overlay = np.zeros((F, H, W), np.int64)
    status = np.zeros((F,), np.int32)
    for f in range(F):
        for p in range(min(max(int(n_points[f]), 0), cap)):
            x, row, col = float(np.float64(points6[f, p, 0])), float(np.float64(points6[f, p, 4])), float(np.float64(points6[f, p, 5]))
            if not (math.isfinite(x) and math.isfinite(row) and math.isfinite(col)):
                continue
            row, col = math.floor(row), math.floor(col)
            dq = clampq(x / float(depth_max) * 65535.0, 65535)
            for rr in range(max(row - R, 0), min(row + R, H - 1) + 1):
                for cc in range(max(col - R, 0), min(col + R, W - 1) + 1):
                    depth[f, rr, cc] = min(depth[f, rr, cc], dq)

    if boxes is not None:
        for f in range(F):
            def segments_of(box, f=f):
                return [tuple((math.floor(e[0]) if math.isfinite(e[0]) else math.nan,
                               math.floor(e[1]) if math.isfinite(e[1]) else math.nan) for e in (p, q))
                        for p, q in camera_endpoints(box, mats[f], float(z_near))]
            _draw_boxes(overlay, status, f, boxes, n_boxes, colors, T, segments_of)
    img = np.zeros((F, H, W, 3), np.uint8)
    lut = np.asarray(lut)
    for f in range(F):
        for r in range(H):
            for c in range(W):
                if overlay[f, r, c]:
                    img[f, r, c] = _rgb(int(overlay[f, r, c]))
                elif depth[f, r, c] != EMPTY:
                    img[f, r, c] = lut[int(depth[f, r, c]) >> 8]
                elif images is not None:
                    img[f, r, c] = images[f, r, c, ::-1] if bgr else images[f, r, c]
    return img, status
