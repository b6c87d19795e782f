"""
Kinematic trees other than synth.icub_like_model(), in the same table form (`wcqp_kin_params`): what the kinematics kernels, the tick's
hand-off choice and the 16-lane walk are run on besides the one iCub-shaped tree.

    one, star26, chain9 / chain17 / chain26, bushy26      random trees: general unit axes, random R0 and frame_R, some links of mass 0,
                                                          root_mass 0, every path plus its frame offset (or link CoM) within 1 m
    icub_gauged, icub_gauged_legs_first, icub_midframe    the iCub-shaped robot in another gauge / numbering / with other frame joints
    icub_interleaved, icub_waist                          the same tree numbered not depth-first; both legs hung under joint 0

`regauge` and `renumber` describe the SAME physical robot in other numbers, `facts` restates what wcqp_kin_create derives from a table
(depth, pointer-jumping rounds, whether subtrees are index ranges, whether the three frame paths are disjoint) without looking at it, so
that a test can assert its tree is of the kind it claims.  Everything is seeded and deterministic.
"""
import functools
import math

import numpy as np

KEYS_PER_JOINT = ("parent", "axis", "p0", "R0", "mass", "com")
LEGS_FIRST = list(range(11, 23)) + list(range(0, 11))
# torso 0 1 2, then the arms' joints alternately (3 7 4 8 ...), then the legs' (11 17 12 18 ...): every parent still precedes its child
INTERLEAVED = [0, 1, 2, 3, 7, 4, 8, 5, 9, 6, 10, 11, 17, 12, 18, 13, 19, 14, 20, 15, 21, 16, 22]


def _copy(model):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in model.items()}


def _rot(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def random_rotations(rng, n):
    """n rotations, uniform axis, angle uniform in +-pi"""
    ax = rng.normal(size=(n, 3))
    return np.stack([_rot(ax[i], rng.uniform(-np.pi, np.pi)) for i in range(n)]) if n else np.zeros((0, 3, 3))


def random_base(rng, count, far=None):
    """[count][12] base poses: position (around 0.5 m up, or around the point `far`), row-major rotation (any)"""
    pos = rng.normal(size=(count, 3)) * 0.05 + (np.array([0.0, 0.0, 0.55]) if far is None else np.asarray(far, float))
    return np.ascontiguousarray(np.concatenate([pos, random_rotations(rng, count).reshape(count, 9)], axis=1))


def random_q(rng, count, dof):
    return np.ascontiguousarray(rng.uniform(-2.0 * np.pi, 2.0 * np.pi, size=(count, dof)))


# ---- the same robot in other numbers ---------------------------------------------------------------------------------------------
def regauge(model, seed):
    """Every joint frame turned by a constant rotation G_j of its own (G = I above the root):
         R0'_j = G_par' R0_j G_j, p0'_j = G_par' p0_j, axis'_j = G_j' axis_j, com'_j = G_j' com_j, frame_R'_f = G_jf' frame_R_f,
         frame_p'_f = G_jf' frame_p_f.
    The world pose of joint frame j becomes R_j G_j at the same origin: axes, link CoMs and attached frames stay where they were."""
    n = int(model["dof"])
    G = random_rotations(np.random.default_rng(seed), n)
    m = _copy(model)
    for j in range(n):
        par = int(model["parent"][j])
        Gp = np.eye(3) if par < 0 else G[par]
        m["R0"][j] = Gp.T @ model["R0"][j] @ G[j]
        m["p0"][j] = Gp.T @ model["p0"][j]
        m["axis"][j] = G[j].T @ model["axis"][j]
        m["com"][j] = G[j].T @ model["com"][j]
    for f in range(3):
        jf = int(model["frame_joint"][f])
        m["frame_R"][f] = G[jf].T @ model["frame_R"][f]
        m["frame_p"][f] = G[jf].T @ model["frame_p"][f]
    return m


def renumber(model, order):
    """New joint k is old joint order[k]: the per-joint arrays permuted, parent and frame_joint remapped."""
    n = int(model["dof"])
    order = [int(x) for x in order]
    assert sorted(order) == list(range(n)), order
    new_of = np.empty(n, np.int64)
    new_of[order] = np.arange(n)
    m = _copy(model)
    for k in KEYS_PER_JOINT:
        m[k] = np.ascontiguousarray(np.asarray(model[k])[order])
    m["parent"] = np.array([-1 if p < 0 else new_of[p] for p in m["parent"]], np.int32)
    m["frame_joint"] = np.array([new_of[int(j)] for j in model["frame_joint"]], np.int32)
    assert all(int(m["parent"][j]) < j for j in range(n)), "a child would precede its parent"
    return m


def permute_joints(array, order):
    """An array over the old joints (q, posture, v_max, joint weights: last axis dof) or a Jacobian (last axis 6 + dof: the base columns
    stay) in the numbering of renumber(model, order)."""
    a = np.asarray(array)
    n = len(order)
    idx = np.asarray(order, np.int64)
    if a.shape[-1] == n:
        return np.ascontiguousarray(a[..., idx])
    assert a.shape[-1] == 6 + n, a.shape
    return np.ascontiguousarray(a[..., np.concatenate([np.arange(6), 6 + idx])])


def unpermute_joints(array, order):
    """the inverse: an array in the numbering of renumber(model, order), back over the old joints"""
    inv = np.empty(len(order), np.int64)
    inv[np.asarray(order, np.int64)] = np.arange(len(order))
    return permute_joints(array, inv)


def scaled_axes(model, factor=3.7):
    """the same table with every axis `factor` long (the library normalises at create; kin_spec does not)"""
    m = _copy(model)
    m["axis"] = m["axis"] * factor
    return m


# ---- what wcqp_kin_create derives from a table, restated ---------------------------------------------------------------------------
def path_to_root(model, j):
    out = []
    j = int(j)
    while j >= 0:
        out.append(j)
        j = int(model["parent"][j])
    return out


def facts(model):
    """depth (joints on the longest path), n_rounds = ceil(log2 depth) of the pointer jumping, dfs_contig (every subtree is an index
    range), disjoint (no joint on two of the three frame paths), paths (the three sets) and handoff: the hand-off the tick takes for
    the tree when nothing is forced."""
    n = int(model["dof"])
    anc = [set(path_to_root(model, j)) for j in range(n)]                    # j and its ancestors
    depth = max(len(a) for a in anc)
    n_rounds = 0 if depth <= 1 else int(math.ceil(math.log2(depth)))
    assert 2 ** n_rounds >= depth and (n_rounds == 0 or 2 ** (n_rounds - 1) < depth)
    dfs_contig = True
    for j in range(n):
        sub = [k for k in range(n) if j in anc[k]]
        dfs_contig = dfs_contig and sub == list(range(j, j + len(sub)))
    paths = [anc[int(j)] for j in model["frame_joint"]]
    disjoint = not (paths[0] & paths[1] or paths[0] & paths[2] or paths[1] & paths[2])
    handoff = "fused" if (disjoint and dfs_contig and n_rounds <= 3 and n == 23) else ("compact" if disjoint else "dense")
    return dict(dof=n, depth=depth, n_rounds=n_rounds, dfs_contig=dfs_contig, disjoint=disjoint, paths=paths, handoff=handoff)


def reach(model):
    """the farthest a point of the robot can be from the root link's origin: path lengths plus the link CoM / frame offset at their end"""
    n = int(model["dof"])
    length = [sum(np.linalg.norm(model["p0"][k]) for k in path_to_root(model, j)) for j in range(n)]
    ends = [length[j] + np.linalg.norm(model["com"][j]) for j in range(n)]
    ends += [length[int(model["frame_joint"][f])] + np.linalg.norm(model["frame_p"][f]) for f in range(3)]
    return max(ends + [np.linalg.norm(model["root_com"])])


# ---- random trees --------------------------------------------------------------------------------------------------------------------
def random_tree(parent, frame_joint, seed):
    """A tree on the given parent table: unit axes in any direction, random R0 / frame_R, links of 0.1 .. 0.3 m, every third link and the
    root link massless, all lengths scaled so that the reach is 0.95 m."""
    rng = np.random.default_rng(seed)
    n = len(parent)
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    unit = lambda k: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(k, 3)))
    mass = rng.uniform(0.2, 3.0, size=n)
    mass[rng.permutation(n)[: n // 3]] = 0.0
    if not mass.any():
        mass[0] = 1.0
    m = dict(dof=n, parent=np.array(parent, np.int32), axis=axis, p0=unit(n) * rng.uniform(0.1, 0.3, size=(n, 1)),
             R0=random_rotations(rng, n), mass=mass, com=unit(n) * rng.uniform(0.0, 0.1, size=(n, 1)),
             root_mass=0.0, root_com=rng.normal(size=3) * 0.05,
             frame_joint=np.array(frame_joint, np.int32), frame_p=unit(3) * rng.uniform(0.02, 0.1, size=(3, 1)),
             frame_R=random_rotations(rng, 3))
    s = 0.95 / reach(m)
    for k in ("p0", "com", "frame_p", "root_com"):
        m[k] = m[k] * s
    assert reach(m) <= 1.0 and m["mass"].sum() + m["root_mass"] > 0
    return m


def _bushy_parents(n, seed):
    """random parents, any earlier joint or the root link - tried seed after seed until the numbering is NOT depth-first and the tree is
    at least five joints deep (deterministic: the first seed that does)"""
    for s in range(seed, seed + 1000):
        rng = np.random.default_rng(s)
        parent = [-1] + [int(rng.integers(-1, j)) for j in range(1, n)]
        f = facts(dict(dof=n, parent=parent, frame_joint=[0, 0, 0]))
        if not f["dfs_contig"] and f["depth"] >= 5:
            return parent
    raise AssertionError("no bushy tree found")


def _icub():
    from walking_controllers_amd import synth
    return synth.icub_like_model()


def _icub_waist():
    """both legs hung under joint 0 (at the place they had: p0 reduced by p0[0]; R0[0] is the identity): joint 0 is on all three frame paths"""
    m = _icub()
    assert np.array_equal(m["R0"][0], np.eye(3))
    for j in (11, 17):
        m["parent"][j] = 0
        m["p0"][j] = m["p0"][j] - m["p0"][0]
    return m


def _icub_midframe():
    """icub_gauged with the left sole on the ankle-pitch joint (15, not the leaf 16) and the neck frame on joint 0"""
    m = named("icub_gauged")
    m["frame_joint"] = np.array([15, 22, 0], np.int32)
    return m


_BUILDERS = {
    "one": lambda: random_tree([-1], [0, 0, 0], 101),
    "star26": lambda: random_tree([-1] * 26, [25, 7, 0], 102),
    "chain9": lambda: random_tree(list(range(-1, 8)), [8, 4, 0], 103),
    "chain17": lambda: random_tree(list(range(-1, 16)), [16, 8, 0], 104),
    "chain26": lambda: random_tree(list(range(-1, 25)), [25, 13, 0], 105),
    "bushy26": lambda: random_tree(_bushy_parents(26, 106), [25, 14, 9], 106),
    "icub_gauged": lambda: regauge(_icub(), 107),
    "icub_gauged_legs_first": lambda: renumber(regauge(_icub(), 107), LEGS_FIRST),
    "icub_interleaved": lambda: renumber(_icub(), INTERLEAVED),
    "icub_waist": _icub_waist,
    "icub_midframe": _icub_midframe,
}
NAMES = list(_BUILDERS)
# what each tree is there for, asserted by the tests through facts(): (n_rounds, dfs_contig, hand-off of the tick left to itself)
CLAIMS = {
    "one": (0, True, "dense"), "star26": (0, True, "compact"), "chain9": (4, True, "dense"), "chain17": (5, True, "dense"),
    "chain26": (5, True, "dense"), "bushy26": (None, False, None), "icub_gauged": (3, True, "fused"),
    "icub_gauged_legs_first": (3, True, "fused"), "icub_interleaved": (3, False, "compact"), "icub_waist": (3, True, "dense"),
    "icub_midframe": (3, True, "fused"),
}
# the numbering of the iCub-shaped variants: new joint k is joint ORDER[name][k] of synth.icub_like_model()
ORDER = {"icub_gauged": list(range(23)), "icub_gauged_legs_first": LEGS_FIRST, "icub_interleaved": INTERLEAVED, "icub_waist": list(range(23)),
         "icub_midframe": list(range(23))}


@functools.lru_cache(maxsize=None)
def _built(name):
    return _BUILDERS[name]()


def named(name):
    """a fresh copy of the named tree"""
    return _copy(_built(name))


def check_claims(name, model=None):
    """assert that the named tree is of the kind it is there for; returns facts()"""
    f = facts(named(name) if model is None else model)
    rounds, contig, handoff = CLAIMS[name]
    assert rounds is None or f["n_rounds"] == rounds, (name, f["n_rounds"])
    assert f["dfs_contig"] == contig, (name, f["dfs_contig"])
    assert handoff is None or f["handoff"] == handoff, (name, f["handoff"])
    return f
