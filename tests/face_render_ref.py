"""An independent NumPy statement of the mesh rasteriser (csrc/face_render_arith.h) and of the vertex colours, and the synthetic meshes
the render tests and tests/golden/make_golden_face_render.py share.

`render` walks the triangles in ascending order with the reference's sequential strict `>` on a float32 depth buffer -- not the 64-bit
key of the library -- and evaluates isPointInTri over a triangle's whole box at once, in float64, one NumPy operation per operation of
render.py:17-41 (NumPy's elementwise products and sums are not fused)."""
import numpy as np

RES = 256
f32, f64 = np.float32, np.float64


def gather(pos, face_ind):
    """One slot's map [256, 256, 3] -> its vertices float32 [V, 3] (get_vertices)."""
    return np.asarray(pos, f32).reshape(RES * RES, 3)[np.asarray(face_ind)]


def place(vertices, face_ind):
    """Vertices [V, 3] -> a map [256, 256, 3] that holds them at the cells face_ind, zeros elsewhere."""
    pos = np.zeros((RES * RES, 3), f32)
    pos[np.asarray(face_ind)] = np.asarray(vertices, f32)
    return pos.reshape(RES, RES, 3)


def render(vertices, triangles, x0, y0, h, w, attrs=None):
    """vertices float32 [V, 3], triangles [T, 3], window (x0, y0, h, w), attrs float32 [V, C] or None (z)
    -> (tri int32 [h, w], image float32 [h, w, C])."""
    v32 = np.asarray(vertices, f32)
    v = v32.astype(f64)
    a = v32[:, 2:3] if attrs is None else np.asarray(attrs, f32)
    C = a.shape[1]
    depth = np.full((h, w), -np.inf, f32)
    tri = np.full((h, w), -1, np.int32)
    image = np.zeros((h, w, C), f32)
    for i, t in enumerate(np.asarray(triangles)):
        p = v[t]
        if not np.isfinite(p).all():
            continue
        with np.errstate(over="ignore"):
            d = f32((p[0, 2] + p[1, 2] + p[2, 2]) / 3.0) + f32(0.0)
        if not d > f32(-999999.0):
            continue
        umin, umax = max(np.ceil(p[:, 0].min()), float(x0)), min(np.floor(p[:, 0].max()), float(x0 + w - 1))
        vmin, vmax = max(np.ceil(p[:, 1].min()), float(y0)), min(np.floor(p[:, 1].max()), float(y0 + h - 1))
        if umax < umin or vmax < vmin:
            continue
        X, Y = np.meshgrid(np.arange(int(umin), int(umax) + 1, dtype=f64), np.arange(int(vmin), int(vmax) + 1, dtype=f64))
        v0, v1 = p[2, :2] - p[0, :2], p[1, :2] - p[0, :2]
        v2x, v2y = X - p[0, 0], Y - p[0, 1]
        dot00, dot01, dot11 = v0[0] * v0[0] + v0[1] * v0[1], v0[0] * v1[0] + v0[1] * v1[1], v1[0] * v1[0] + v1[1] * v1[1]
        dot02, dot12 = v0[0] * v2x + v0[1] * v2y, v1[0] * v2x + v1[1] * v2y
        det = dot00 * dot11 - dot01 * dot01
        inv = 0.0 if det == 0 else 1.0 / det
        bu, bv = (dot11 * dot02 - dot01 * dot12) * inv, (dot00 * dot12 - dot01 * dot02) * inv
        take = (bu >= 0) & (bv >= 0) & (bu + bv < 1)
        rows, cols = (Y[take] - y0).astype(int), (X[take] - x0).astype(int)
        win = d > depth[rows, cols]
        rows, cols = rows[win], cols[win]
        depth[rows, cols], tri[rows, cols] = d, i
        aa = a[t].astype(f64)
        with np.errstate(over="ignore", invalid="ignore"):
            image[rows, cols] = ((aa[0] + aa[1] + aa[2]) / 3.0).astype(f32)
    return tri, image


def render_slots(pos, slots, face_ind, triangles, origin, h, w, attrs=None):
    """The call over every slot -> (tri [cap, h, w], image [cap, h, w, C]); unused slots and origins beyond +-2^20 give -1 / 0."""
    cap = len(slots)
    C = 1 if attrs is None else attrs.shape[2]
    tri, image = np.full((cap, h, w), -1, np.int32), np.zeros((cap, h, w, C), f32)
    for s in range(cap):
        if slots[s] < 0 or np.abs(np.asarray(origin[s], np.int64)).max() > 1 << 20:
            continue
        tri[s], image[s] = render(gather(pos[s], face_ind), triangles, int(origin[s][0]), int(origin[s][1]), h, w,
                                  None if attrs is None else attrs[s])
    return tri, image


def vertex_colors(pictures, pos, slots, face_ind):
    """pictures: N arrays [H, W, 3] in B, G, R -> float32 [cap, V, 3] (PRN.get_colors, prnet.py:155-168): np.round of the clamped x, y."""
    cap, N = len(slots), len(pictures)
    q = cap // N
    out = np.zeros((cap, len(face_ind), 3), f32)
    for s in range(cap):
        if slots[s] < 0 or s // q >= N:
            continue
        pic = pictures[s // q]
        H, W = pic.shape[:2]
        v = gather(pos[s], face_ind).astype(f64)
        ok = np.isfinite(v[:, 0]) & np.isfinite(v[:, 1])
        x = np.round(np.clip(np.where(ok, v[:, 0], 0.0), 0, W - 1)).astype(int)
        y = np.round(np.clip(np.where(ok, v[:, 1], 0.0), 0, H - 1)).astype(int)
        out[s] = np.where(ok[:, None], pic[y, x].astype(f32), f32(0))
    return out


# ---- synthetic meshes ------------------------------------------------------------------------------------------------------------------
def block_ind(G, row0=100, col0=90):
    """face_ind of a G x G block of map cells, row-major."""
    r, c = np.meshgrid(np.arange(row0, row0 + G), np.arange(col0, col0 + G), indexing="ij")
    return (r * RES + c).reshape(-1).astype(np.int32)


def cap_mesh(seed, G, turn, noise, centre, radius):
    """float32 [G * G, 3]: a G x G grid over an ellipsoid cap, every point moved by uniform noise, turned by `turn` rad about the y axis
    (and a third of it about x) so that the surface folds over itself, then moved to `centre` = (x, y, z)."""
    r = np.random.RandomState(seed)
    a, b = np.meshgrid(np.linspace(-1.0, 1.0, G), np.linspace(-1.0, 1.0, G))
    p = np.stack([a * radius, b * radius * 1.15, np.sqrt(np.maximum(0.0, 1.0 - 0.8 * (a * a + b * b))) * radius * 2.3], -1).reshape(-1, 3)
    p = p + r.uniform(-noise, noise, p.shape)
    cy, sy, cx, sx = np.cos(turn), np.sin(turn), np.cos(turn / 3.0), np.sin(turn / 3.0)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return (p @ (Rx @ Ry).T + np.asarray(centre, f64)).astype(f32)


def fuzz_mesh(seed, V, T, h, w, x0=0, y0=0):
    """(vertices float32 [V, 3], triangles int32 [T, 3]) that take every branch of the rule: small triangles over the window, some far
    larger than it, some wholly outside, degenerate ones (a repeated vertex, three collinear points: the whole box is covered), exact
    duplicates of earlier triangles (the lower index wins), depths of +0 / -0 and at or below -999999, vertices with NaN / inf and with
    coordinates of +-1e30."""
    r = np.random.RandomState(seed)
    v = np.empty((V, 3), f64)
    k = np.arange(V) * 1.7                                        # a serpentine over the window: neighbours in the list lie close
    v[:, 0] = x0 - 4 + k % (w + 8) + r.uniform(-0.8, 0.8, V)
    v[:, 1] = y0 - 4 + (k // (w + 8)) * (h + 8.0) / max(1.0, k[-1] // (w + 8)) + r.uniform(-1.2, 1.2, V)
    v[:, 2] = r.uniform(-30, 30, V).round(1)
    whole = r.rand(V) < 0.3
    v[whole, :2] = np.round(v[whole, :2])                         # vertices on pixel centres: u, v and u + v of exactly 0 and 1
    v[:8, 2] = [0.0, -0.0, 0.0, -0.0, -999999.0, -1e6, -3e6, 0.0]
    v[8] = (np.nan, y0 + 3, 1.0)
    v[9] = (x0 + 2, np.inf, 1.0)
    v[10] = (x0 + 2, y0 + 2, -np.inf)
    v[11] = (1e30, y0 + 5, 2.0)
    v[12] = (x0 + 5, -1e30, 2.0)
    v[13] = (-1e30, 1e30, 3.0)
    v[14] = (x0 - 300.0, y0 - 200.0, 4.0)
    v[15] = (x0 + w + 400.0, y0 - 100.0, 4.0)
    v[16] = (x0 + w / 2.0, y0 + h + 500.0, 4.0)
    tri = np.empty((T, 3), np.int32)
    for i in range(T):
        kind = r.randint(0, 12)
        a = r.randint(17, V)
        near = 17 + (a - 17 + r.randint(1, 6, 2)) % (V - 17)
        if kind == 0:
            tri[i] = r.randint(0, V, 3)                            # anything, the special vertices included
        elif kind == 1:
            tri[i] = (a, a, near[0])                               # degenerate: a repeated vertex
        elif kind == 2 and i > 0:
            tri[i] = tri[r.randint(0, i)]                          # an exact duplicate
        elif kind == 3:
            tri[i] = (r.randint(0, 8), r.randint(0, 8), r.randint(0, 8))   # depths of +-0 and below the floor
        elif kind == 4:
            tri[i] = (14, 15, 16) if r.rand() < 0.5 else (r.randint(11, 17), a, near[0])     # huge
        else:
            tri[i] = (a, near[0], near[1])
    # three collinear points with a box of several pixels
    v[17], v[18], v[19] = (x0 + 1, y0 + 1, 5.0), (x0 + 3, y0 + 2, 5.0), (x0 + 5, y0 + 3, 5.0)
    tri[0] = (17, 18, 19)
    return v.astype(f32), tri
