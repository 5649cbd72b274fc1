"""What the head-pose tests share on the library's side: the call of the HOST twin (cp_face_pose_host) over guarded arrays, synthetic
plan outputs with their slots and crop squares, and the fixture."""
import ctypes
import functools
import os

import numpy as np

import face_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64            # elements behind every output that no call may touch
SENTINEL = -7.25      # what the scratch holds before a call (an unused slot's part stays so)
NMOM, CHUNK = 13, 2048
SIZES = dict(P=12, angles=3, scale=1, box=20, valid=1)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "face_pose.npz")))


def scratch_doubles(cap, V):
    return cap * (-(-V // CHUNK) * NMOM + 3)


def outputs(cap, V):
    """Guarded, sentinel-filled output arrays of one call: name -> flat array."""
    out = {k: np.full(n * cap + GUARD, SENTINEL if k in ("P", "angles", "scale") else -7, np.int32 if k in ("box", "valid") else np.float64)
           for k, n in SIZES.items()}
    out["scratch"] = np.full(scratch_doubles(cap, V) + GUARD, SENTINEL, np.float64)
    return out


def guards_intact(out, cap, V):
    ok = all((out[k][n * cap:] == (SENTINEL if out[k].dtype == np.float64 else -7)).all() for k, n in SIZES.items())
    return ok and (out["scratch"][scratch_doubles(cap, V):] == SENTINEL).all()


def shaped(out, cap):
    return dict(P=out["P"][:12 * cap].reshape(cap, 3, 4), angles=out["angles"][:3 * cap].reshape(cap, 3), scale=out["scale"][:cap],
                box=out["box"][:20 * cap].reshape(cap, 10, 2), valid=out["valid"][:cap], scratch=out["scratch"])


def host_pose(L, src, from_pos, slots, xform, face_ind, centred, stats, landmarks, scratch_bytes=None):
    """-> (rc, dict of P [cap, 3, 4], angles, scale, box, valid and the whole guarded scratch); guards checked."""
    cap, V = len(slots), len(face_ind)
    a = [np.ascontiguousarray(src, np.float32), np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(xform, np.float32),
         np.ascontiguousarray(face_ind, np.int32), np.ascontiguousarray(centred, np.float64), np.ascontiguousarray(stats, np.float64),
         np.ascontiguousarray(landmarks, np.float32)]
    out = outputs(cap, V)
    p = lambda x: x.ctypes.data
    rc = L.cp_face_pose_host(p(a[0]), int(from_pos), p(a[1]), p(a[2]), cap, p(a[3]), V, p(a[4]), p(a[5]), p(a[6]), p(out["scratch"]),
                             scratch_doubles(cap, V) * 8 if scratch_bytes is None else scratch_bytes, p(out["P"]), p(out["angles"]),
                             p(out["scale"]), p(out["box"]), p(out["valid"]))
    assert guards_intact(out, cap, V)
    return rc, shaped(out, cap)


def synthetic(seed, cap, used, x0_max=8000.0):
    """Random plan outputs [cap, 3, 256, 256] in 0..1 with slots (-1 where not `used`) and crop squares with x0 up to x0_max."""
    r = np.random.RandomState(seed)
    net = r.random_sample((cap, 3, 256, 256)).astype(np.float32)
    slots = np.asarray([s if s in used else -1 for s in range(cap)], np.int32)
    xform = np.zeros((cap, 3), np.float32)
    for s in used:
        xform[s] = (r.uniform(-300.0, x0_max) if s else x0_max, r.uniform(-300.0, 2000.0), float(r.randint(20, 900)))
    return net, slots, xform


def restored(L, net, slots, xform, uv=None):
    """(pos [cap, 256, 256, 3], landmarks [cap, 68, 3]) by the restore's host twin."""
    rc, pos, lm = face_util.host_restore(L, net, slots, xform, face_util.uv_table() if uv is None else uv)
    assert rc == 0
    return pos, lm


def same_bits64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
