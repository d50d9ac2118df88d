"""Raster flood fill in plain numpy / Python: the connected components, their first pixels and the twelve integers of include/mi355seg.h
(mi_label_components, mi_lesion_score) from the definitions alone.  Shares nothing with the kernels or with host/metrics.py.  Also the input cases
of tests/test_host_components.py and tests/test_gpu_components.py."""
import numpy as np

INTS = 12
STEPS = {4: ((-1, 0), (0, -1), (0, 1), (1, 0)),
         8: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def label(mask, connectivity):
    """mask bool [H, W] -> (labels int32 [H, W]: 0 on background, else 1..n in the raster order of each component's first pixel; roots int32
    [H, W]: the linear index of that first pixel, -1 on background; n)."""
    m = np.asarray(mask, dtype=bool)
    H, W = m.shape
    steps = STEPS[connectivity]
    labels, roots = np.zeros((H, W), np.int32), np.full((H, W), -1, np.int32)
    n = 0
    fg = m.tolist()
    seen = [[False] * W for _ in range(H)]
    for y0 in range(H):
        for x0 in range(W):
            if not fg[y0][x0] or seen[y0][x0]:
                continue
            n += 1
            seen[y0][x0] = True
            stack, ys, xs = [(y0, x0)], [], []
            while stack:
                y, x = stack.pop()
                ys.append(y)
                xs.append(x)
                for dy, dx in steps:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and fg[v][u] and not seen[v][u]:
                        seen[v][u] = True
                        stack.append((v, u))
            labels[ys, xs] = n
            roots[ys, xs] = y0 * W + x0
    return labels, roots, n


def _areas(labels, n):
    return np.bincount(labels.ravel(), minlength=n + 1)


def _overlaps(hit, area, permille):
    return int(hit) >= 1 and 1000 * int(hit) >= int(permille) * int(area)


def reference(pred, lab, cls=1, connectivity=8, min_area=0, keep_largest=False, permille=0):
    """One image.  Returns (ints int64 [12] as mi_lesion_score lays them out, filtered uint8 [H, W])."""
    P, G = np.asarray(pred) == cls, np.asarray(lab) == cls
    lp, _, n_p = label(P, connectivity)
    lg, _, n_g = label(G, connectivity)
    area_p, area_g = _areas(lp, n_p), _areas(lg, n_g)
    kept = [k for k in range(1, n_p + 1) if area_p[k] >= min_area]
    if keep_largest and kept:
        kept = [max(kept, key=lambda k: (area_p[k], -k))]              # numbers follow the first pixels: a tie goes to the smaller number
    F = np.isin(lp, kept) & P
    tp = sum(1 for k in kept if _overlaps((G & (lp == k)).sum(), area_p[k], permille))
    det = sum(1 for k in range(1, n_g + 1) if _overlaps((F & (lg == k)).sum(), area_g[k], permille))
    ints = np.array([P.sum(), F.sum(), G.sum(), n_p, len(kept), n_g, tp, det, area_p[1:].max() if n_p else 0, area_g[1:].max() if n_g else 0,
                     (F & G).sum(), n_p - len(kept)], np.int64)
    filtered = np.where(F, cls, 1 if cls == 0 else 0).astype(np.uint8)
    return ints, filtered


# ------------------------------------------------------------------------------------------------ the cases
def ellipse(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) < 1).astype(np.uint8)


def speckle(H, W, share, seed):
    return (np.random.RandomState(seed).rand(H, W) < share).astype(np.uint8)


def words(W):
    """1 x W, all foreground, with one hole at x = 64 where W allows: runs ending at, starting at and crossing a 64-lane ballot word."""
    m = np.ones((1, W), np.uint8)
    if W > 64:
        m[0, 64] = 0
    return m


def u_shape():
    """6 x 9: two arms that join on the LAST row (one component, number 1), a pixel between them, and a diagonal pair (one component under
    connectivity 8, two under 4)."""
    m = np.zeros((6, 9), np.uint8)
    m[:, 0] = m[:, 4] = m[5, 0:5] = 1
    m[2, 2] = 1
    m[1, 6] = m[2, 7] = 1
    return m


def spiral(H, W):
    """A one-pixel-wide spiral from pixel 0 inwards, one background pixel between its turns.  Returns (mask, number of turns)."""
    m = np.zeros((H, W), np.uint8)
    y = x = k = turns = 0
    m[0, 0] = 1
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(v, u):
        return not (0 <= v < H and 0 <= u < W) or m[v, u] == 0

    def can(dy, dx):
        v, u = y + dy, x + dx
        return 0 <= v < H and 0 <= u < W and m[v, u] == 0 and free(v + dy, u + dx)

    while True:
        if not can(*dirs[k]):
            k = (k + 1) % 4
            if not can(*dirs[k]):
                return m, turns
            turns += 1
        y, x = y + dirs[k][0], x + dirs[k][1]
        m[y, x] = 1


def checker(H, W):
    return (np.add.outer(np.arange(H), np.arange(W)) % 2 == 0).astype(np.uint8)


def comb(H, W):
    """Teeth on every even column, joined by the LAST row only: every union happens at the bottom."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = 1
    m[H - 1, :] = 1
    return m


def frames(H, W, n=4, step=3):
    """n nested one-pixel rings, `step` apart: they touch under neither connectivity."""
    m = np.zeros((H, W), np.uint8)
    for k in range(n):
        o = k * step
        m[o, o:W - o] = m[H - 1 - o, o:W - o] = 1
        m[o:H - o, o] = m[o:H - o, W - 1 - o] = 1
    return m


def blobs(H, W, seed):
    m = ellipse(H, W, 60, 70, 40, 50) | ellipse(H, W, 130, 440, 50, 60) | ellipse(H, W, 150, 250, 20, 64)
    return m | speckle(H, W, 0.02, seed)


def label_cases():
    """name -> mask uint8 [H, W] with values in {0, 1}."""
    out = {"words_1x%d" % W: words(W) for W in (1, 63, 64, 65, 130)}
    out["u_shape_6x9"] = u_shape()
    out["spiral_33x64"] = spiral(33, 64)[0]
    out["checker_37x45"] = checker(37, 45)
    out["comb_40x130"] = comb(40, 130)
    out["frame_in_frame_37x45"] = frames(37, 45)
    out["speckle_37x45"] = speckle(37, 45, 0.45, 1)
    out["blobs_200x517"] = blobs(200, 517, 2)
    out["full_9x70"] = np.ones((9, 70), np.uint8)
    out["empty_9x70"] = np.zeros((9, 70), np.uint8)
    single = np.zeros((9, 70), np.uint8)
    single[4, 66] = 1
    out["single_9x70"] = single
    return out


def lesion_cases():
    """name -> (pred uint8 [H, W], label int64 [H, W]) at 37 x 80."""
    H, W = 37, 80
    out = {}

    def add(name, p, g):
        out[name] = (np.ascontiguousarray(p, dtype=np.uint8), np.ascontiguousarray(g).astype(np.int64))

    a, b = ellipse(H, W, 12, 20, 8, 12), ellipse(H, W, 24, 58, 9, 14)
    add("shifted", np.roll(a, 5, axis=1) | np.roll(b, -4, axis=0), a | b)
    specks = np.zeros((H, W), np.uint8)
    specks[2, 70] = specks[3, 71] = 1                                   # a diagonal pair: area 2 under connectivity 8, twice area 1 under 4
    specks[30:33, 3:7] = 1                                              # area 12, no lesion under it
    specks[23:26, 43:47] = 1                                            # area 12, exactly half of it inside the second lesion's left rim
    specks[35, 40:75] = 1                                               # area 35
    add("specks", a | specks, a | b)
    add("split", ellipse(H, W, 18, 25, 6, 7) | ellipse(H, W, 18, 55, 6, 7), ellipse(H, W, 18, 40, 10, 30))      # one lesion, two predictions on it
    add("bridge", ellipse(H, W, 18, 40, 5, 30), ellipse(H, W, 18, 18, 9, 9) | ellipse(H, W, 18, 62, 9, 9))     # one prediction over two lesions
    tie = np.zeros((H, W), np.uint8)
    tie[4:8, 60:66] = 1                                                 # two components of 24 pixels: the first in raster order wins
    tie[20:26, 10:14] = 1
    tie[30, 30:40] = 1
    add("tie", tie, np.roll(tie, 2, axis=1))
    return out


def multi_class_map(H, W, seed):
    """A map with the values 0..4 in blocks plus noise, for cls = 3."""
    g = np.random.RandomState(seed)
    m = (np.add.outer(np.arange(H) // 7, np.arange(W) // 9) % 5).astype(np.int64)
    noise = g.rand(H, W) < 0.05
    m[noise] = g.randint(0, 5, int(noise.sum()))
    return m
