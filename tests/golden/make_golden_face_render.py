"""Records tests/golden/face_render.npz from the reference's own renderer (demo/face/utils/render.py), imported by path:

    python tests/golden/make_golden_face_render.py [path of the reference checkout]

(default: $CP_REFERENCE, or a directory `reference` beside the repository).  The file holds three synthetic meshes (tests/face_render_ref.py:
a 24 x 24 grid over an ellipsoid cap with uniform noise, turned far enough that the surface folds over itself; triangles by
face.grid_triangles) as float32 vertices with random float32 colours, and what the reference computes for each in a 40 x 48 window:
get_triangle_buffer, render_texture with the vertices' z (c = 1) and with the colours (c = 3), fed FLOAT64 COPIES of the float32 arrays
(the reference's vertices are float64).  Cases 0 and 1 are rendered in a frame that is the window; case 2 in a 64 x 72 frame and cropped to
the window at (9, 13): the library clamps a triangle's box to the window, the reference to the frame.

Asserted here, on the reference alone, so that no test has to leave a pixel out: every (triangle, box pixel) pair has
min(|u|, |v|, |1 - u - v|) >= 1e-6, any two triangles that cover one pixel differ in depth by >= 1e-3 (far above the float32 rounding of
the library's key), no triangle is degenerate, and at least a fifth of the covered pixels lie under more than one triangle."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import face_render_ref as ref  # noqa: E402

G, H, W = 24, 40, 48
# (seed, turn, frame (h, w), origin (x0, y0))
CASES = [(4100, 0.7, (H, W), (0, 0)), (4101, -1.0, (H, W), (0, 0)), (4102, 1.25, (64, 72), (9, 13))]
NOISE, RADIUS = 0.2, 13.0


def margins(v, tri, fh, fw):
    """-> (smallest min(|u|, |v|, |1 - u - v|) over all (triangle, box pixel) pairs, smallest depth gap between two triangles covering one
    pixel, pairs, covered pixels, pixels under more than one triangle); float64, the reference's operation order."""
    edge, pairs = np.inf, 0
    cover = [[[] for _ in range(fw)] for _ in range(fh)]
    for i, t in enumerate(tri):
        p = v[t]
        umin, umax = max(int(np.ceil(p[:, 0].min())), 0), min(int(np.floor(p[:, 0].max())), fw - 1)
        vmin, vmax = max(int(np.ceil(p[:, 1].min())), 0), min(int(np.floor(p[:, 1].max())), fh - 1)
        v0, v1 = p[2, :2] - p[0, :2], p[1, :2] - p[0, :2]
        dot00, dot01, dot11 = np.dot(v0, v0), np.dot(v0, v1), np.dot(v1, v1)
        det = dot00 * dot11 - dot01 * dot01
        assert det != 0, ("degenerate triangle", i)
        d = (p[0, 2] + p[1, 2] + p[2, 2]) / 3.0
        for x in range(umin, umax + 1):
            for y in range(vmin, vmax + 1):
                v2 = np.array([x, y], np.float64) - p[0, :2]
                dot02, dot12 = np.dot(v0, v2), np.dot(v1, v2)
                bu, bv = (dot11 * dot02 - dot01 * dot12) / det, (dot00 * dot12 - dot01 * dot02) / det
                edge, pairs = min(edge, abs(bu), abs(bv), abs(1 - bu - bv)), pairs + 1
                if bu >= 0 and bv >= 0 and bu + bv < 1:
                    cover[y][x].append(d)
    gap, covered, multi = np.inf, 0, 0
    for row in cover:
        for ds in row:
            covered, multi = covered + (len(ds) > 0), multi + (len(ds) > 1)
            s = np.sort(ds)
            if len(s) > 1:
                gap = min(gap, np.diff(s).min())
    return edge, gap, pairs, covered, multi


def main():
    from centerpose_amd import face
    reference = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CP_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
    spec = importlib.util.spec_from_file_location("reference_render", os.path.join(reference, "demo", "face", "utils", "render.py"))
    rr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rr)

    face_ind = ref.block_ind(G)
    tri = face.grid_triangles(face_ind)
    assert tri.shape == (2 * (G - 1) ** 2, 3)
    out = {k: [] for k in ("vertices", "colors", "origin", "tri", "depth", "texture")}
    worst_edge, worst_gap, shares = np.inf, np.inf, []
    for seed, turn, (fh, fw), (x0, y0) in CASES:
        v32 = ref.cap_mesh(seed, G, turn, NOISE, (x0 + W / 2.0 + 0.3, y0 + H / 2.0 - 0.4, 40.0), RADIUS)
        c32 = np.random.RandomState(seed + 50).uniform(0.0, 255.0, v32.shape).astype(np.float32)
        v64, c64 = v32.astype(np.float64), c32.astype(np.float64)
        edge, gap, pairs, covered, multi = margins(v64, tri, fh, fw)
        assert edge >= 1e-6 and gap >= 1e-3 and multi >= 0.2 * covered, (seed, edge, gap, covered, multi)
        worst_edge, worst_gap = min(worst_edge, edge), min(worst_gap, gap)
        shares.append((pairs, covered, multi))
        crop = (slice(y0, y0 + H), slice(x0, x0 + W))
        buf = rr.get_triangle_buffer(v64.T, tri.T, fh, fw)[crop]
        depth = rr.render_texture(v64.T, v64[:, 2:3].T, tri.T, fh, fw, c=1)[crop]
        tex = rr.render_texture(v64.T, c64.T, tri.T, fh, fw, c=3)[crop]
        assert buf.dtype == np.int32 and depth.shape == (H, W, 1) and tex.shape == (H, W, 3)
        for key, val in (("vertices", v32), ("colors", c32), ("origin", (x0, y0)), ("tri", buf), ("depth", depth.astype(np.float32)),
                         ("texture", tex.astype(np.float32))):
            out[key].append(val)
    arrays = {k: np.asarray(v) for k, v in out.items()}
    arrays["origin"] = arrays["origin"].astype(np.int32)
    path = os.path.join(HERE, "face_render.npz")
    np.savez_compressed(path, face_ind=face_ind, size=np.asarray([H, W], np.int32), **arrays)
    size = os.path.getsize(path)
    assert size <= 225 * 1024, size
    print("face_render.npz: %d bytes, %d cases; barycentrics >= %.2e from an edge, depth gaps >= %.3f; (pairs, covered, under several): %s"
          % (size, len(CASES), worst_edge, worst_gap, shares))


if __name__ == "__main__":
    main()
