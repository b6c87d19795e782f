"""Set-based checks of support-polygon rows (include/wcqp.h, hull section) and the foot-pose families they are pointed at
(tests/test_hull_stances.py).  Pure numpy.

With parallel feet several corners lie on one line, the monotone chain's orientation test then decides on rounding, and a builder may
deliver an edge once or twice: the row COUNT is not a function of the polygon.  So rows are compared as sets (same_polygon), or against
the corners themselves (contains_and_supports), never index by index."""
import numpy as np

from walking_controllers_amd import synth

HULL_ROWS = 8
HULL_PAD_B = 1e30
FAMILIES = ("side", "axis", "tandem", "stagger", "overlap", "tilt", "same")


def _rows(A, b):
    return np.asarray(A, float).reshape(-1, 2), np.asarray(b, float).reshape(-1)


def row_gaps(A, b, nc, A_ref, b_ref, nc_ref):
    """For every row k < nc the reference row closest to it: (|dA|_inf [nc], |db| [nc], its index [nc]); closest in the larger of the two
    gaps, each in units of the polygon bars (1e-9 for the normal, 1e-12 for the offset)."""
    A, b = _rows(A, b)
    Ar, br = _rows(A_ref, b_ref)
    dA = np.abs(A[:nc, None, :] - Ar[None, :nc_ref, :]).max(-1)
    db = np.abs(b[:nc, None] - br[None, :nc_ref])
    j = np.argmin(np.maximum(dA / 1e-9, db / 1e-12), axis=1)
    k = np.arange(nc)
    return dA[k, j], db[k, j], j


def polygon_diff(A, b, nc, A_ref, b_ref, nc_ref, tol_a=1e-9, tol_b=1e-12) -> str:
    """Why the rows (A, b, nc) are not the polygon of (A_ref, b_ref, nc_ref); "" when they are.  See same_polygon."""
    A, b = _rows(A, b)
    nc, nc_ref = int(nc), int(nc_ref)
    if not (0 <= nc <= HULL_ROWS and len(b) == HULL_ROWS and A.shape == (HULL_ROWS, 2)):
        return "shape / row count out of range: nc %d" % nc
    if not (np.all(A[nc:] == 0.0) and np.all(b[nc:] == HULL_PAD_B)):
        return "rows at and above nc = %d are not the padding 0.u <= 1e30" % nc
    if not (np.all(np.isfinite(A[:nc])) and np.all(np.isfinite(b[:nc]))):
        return "non-finite row below nc = %d" % nc
    if nc == 0 or nc_ref == 0:
        return "" if nc == nc_ref else "nc %d against the reference's %d" % (nc, nc_ref)
    err = np.abs(np.hypot(A[:nc, 0], A[:nc, 1]) - 1.0).max()
    if err > 1e-12:
        return "a normal is not of unit length: off by %.3g" % err
    # the normals turn counter-clockwise, once around: every step of the angle >= 0 (a repeated edge: ~0), the steps sum to one turn
    ang = np.arctan2(A[:nc, 1], A[:nc, 0])
    # (taken into [-tol_a, 2 pi - tol_a): a step back by more than tol_a counts as almost a whole turn, and the sum gives it away)
    step = np.mod(np.roll(ang, -1) - ang + tol_a, 2.0 * np.pi) - tol_a
    if nc >= 2 and abs(step.sum() - 2.0 * np.pi) > 1e-9 * nc:
        return "the normals do not turn counter-clockwise once around: steps %s" % np.array2string(step, precision=3)
    for x, y, what in (((A, b, nc), (A_ref, b_ref, nc_ref), "row %d matches no reference row"), ((A_ref, b_ref, nc_ref), (A, b, nc), "reference row %d is matched by no row")):
        dA, db, j = row_gaps(*x, *y)
        bad = np.nonzero((dA > tol_a) | (db > tol_b))[0]
        if bad.size:
            k = int(bad[0])
            return (what % k) + ": closest is %d at |dA| %.3g |db| %.3g" % (int(j[k]), dA[k], db[k])
    return ""


def same_polygon(A, b, nc, A_ref, b_ref, nc_ref, tol_a=1e-9, tol_b=1e-12) -> bool:
    """The rows (A[8][2], b[8], nc) describe the polygon of the reference rows, as sets: every row below nc matches some reference row
    within tol_a in the normal and tol_b in the offset and every reference row is matched by a row below nc (an edge may repeat on either
    side); rows below nc are finite with unit normals to 1e-12, their angles non-decreasing around the circle with one wrap; rows at and
    above nc are the padding, A == 0 and b == 1e30 exactly.  tol_b = 1e-12 is the hull bar of test_hull_rows_from_foot_poses, tol_a = 1e-9
    the parity bar and the MPC's parallel-row threshold.  polygon_diff says why not."""
    return polygon_diff(A, b, nc, A_ref, b_ref, nc_ref, tol_a, tol_b) == ""


def support_diff(A, b, nc, points, tol=1e-12) -> str:
    A, b = _rows(A, b)
    P = np.asarray(points, float).reshape(-1, 2)
    if not (np.all(np.isfinite(A[:nc])) and np.all(np.isfinite(b[:nc]))):
        return "non-finite row below nc = %d" % nc
    if nc == 0:
        return "no rows"
    res = P @ A[:nc].T - b[:nc][None, :]                  # [point][row], <= 0 inside
    if res.max() > tol:
        return "corner %d violates row %d by %.3g" % (*np.unravel_index(np.argmax(res), res.shape), res.max())
    loose = np.abs(res).min(axis=0)
    if loose.max() > tol:
        return "row %d is tight at no corner: nearest at %.3g" % (int(np.argmax(loose)), loose.max())
    return ""


def contains_and_supports(A, b, nc, points, tol=1e-12) -> bool:
    """Every corner of `points` [n][2] satisfies every row below nc, and every row is tight at some corner, to tol.  Needs no reference."""
    return support_diff(A, b, nc, points, tol) == ""


def minimal_rows(A, b, nc, tol_a=1e-9, tol_b=1e-12):
    """(A[8][2], b[8], nc) with the rows that same_polygon would call equal merged into the first of them, order kept, padded."""
    A, b = _rows(A, b)
    keep = []
    for k in range(int(nc)):
        if not any(np.abs(A[k] - A[j]).max() <= tol_a and abs(b[k] - b[j]) <= tol_b for j in keep):
            keep.append(k)
    Am = np.zeros((HULL_ROWS, 2)); bm = np.full(HULL_ROWS, HULL_PAD_B)
    Am[:len(keep)] = A[keep]; bm[:len(keep)] = b[keep]
    return Am, bm, len(keep)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1.0, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def pose(xy, R):
    """[12]: position (x, y, 0), row-major rotation"""
    return np.concatenate([np.asarray(xy, float), [0.0], np.asarray(R, float).reshape(9)])


def stances(name: str, n: int, seed: int):
    """(left_T [n][12], right_T [n][12]): n robots of one family of foot poses, deterministic in (name, n, seed), the feet's midpoint within
    5 cm of the origin, for the rectangle synth.FOOT_RECT.  `long` is the foot's x axis (its heading), `lat` the y axis (left is +lat).
      side     parallel feet side by side, 0.1 .. 0.2 m apart laterally, any yaw: front and back edges collinear, the hull a rectangle
      axis     the same at a yaw of 0, +-pi/2 or pi
      tandem   the same yaw, one foot 0.08 .. 0.2 m ahead of the other: the side edges collinear
      stagger  parallel, 0.16 m apart laterally, the left foot 0.1 m ahead or behind: a hexagon, no three corners on a line
      overlap  centres 0.01 m apart, yaws up to 1 rad apart
      tilt     side by side with a roll and a pitch of up to +-0.5 rad on each foot and independent yaws
      same     both feet at one pose"""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    L, R = np.zeros((n, 12)), np.zeros((n, 12))
    for i in range(n):
        mid = rng.uniform(-0.05, 0.05, 2)
        yaw = rng.uniform(-np.pi, np.pi)
        u = rng.uniform(0.0, 1.0, 8)
        if name == "axis":
            yaw = (0.0, 0.5 * np.pi, -0.5 * np.pi, np.pi)[i % 4]
        Rl = Rr = _rot("z", yaw)
        long_, lat = Rl[:2, 0], Rl[:2, 1]
        if name in ("side", "axis"):
            off = 0.5 * (0.1 + 0.1 * u[0]) * lat
        elif name == "tandem":
            off = 0.5 * (0.08 + 0.12 * u[0]) * long_ * (1.0 if u[1] < 0.5 else -1.0)
        elif name == "stagger":
            off = 0.08 * lat + 0.05 * long_ * (1.0 if u[1] < 0.5 else -1.0)
        elif name == "overlap":
            a = 2.0 * np.pi * u[0]
            off = 0.005 * np.array([np.cos(a), np.sin(a)])
            Rr = _rot("z", yaw + 2.0 * u[1] - 1.0)
        elif name == "tilt":
            off = 0.5 * (0.1 + 0.1 * u[0]) * lat
            Rl = _rot("z", yaw) @ _rot("y", u[1] - 0.5) @ _rot("x", u[2] - 0.5)
            Rr = _rot("z", yaw + 0.6 * u[3] - 0.3) @ _rot("y", u[4] - 0.5) @ _rot("x", u[5] - 0.5)
        elif name == "same":
            off = np.zeros(2)
        else:
            raise ValueError(name)
        L[i], R[i] = pose(mid + off, Rl), pose(mid - off, Rr)
    return L, R


def corners(left_T, right_T, contact: int, rect=None) -> np.ndarray:
    """The projected corners [4 or 8][2] of the feet in contact (bit 0 left, bit 1 right), by the oracle's own projection."""
    from oracle import hull_spec as hs
    rect = synth.FOOT_RECT if rect is None else rect
    return np.vstack([hs.foot_points(rect, T) for bit, T in ((1, left_T), (2, right_T)) if contact & bit])
