"""Worlds for the function-level XPBD solver tests (test_solver_functions*.py).

Pure numpy, seeded, deterministic.  A world is the flat description that
oracle/ref_shims/xpbd_ref_shim.cpp documents (bodies 48 floats, contacts 20
floats + 3 ints, joints 20 floats + 3 ints, sys 5 floats).  Every family is
built by construction so that the branch it names is certain to be taken.
"""
import ctypes as C

import numpy as np

F = np.float32
BODY_STRIDE = 48
BODY_STATE = 33
CONTACT_STRIDE = 20
JOINT_STRIDE = 20
MAX_BODIES = 24
DYNAMIC, KINEMATIC, STATIC = 0, 1, 2
FIXED, HINGE = 0, 1
ALL_MASKS = tuple(range(1, 32))
H = F(1.0 / 240.0)
GRAVITY = (0.0, 0.0, -9.8)
THRESHOLD = F(0.05)     # 2 |g| h is ~0.08 in the simulators


class World:
    def __init__(self, tag):
        self.tag = tag
        self.bodies = []
        self.types = []
        self.contacts = []
        self.cints = []
        self.joints = []
        self.jints = []
        self.lambdas = []
        self.sys = np.array([H, *GRAVITY, THRESHOLD], F)

    # -- bodies ----------------------------------------------------------------
    def add_body(self, row, kind=DYNAMIC, limit=MAX_BODIES):
        assert len(self.bodies) < limit
        self.bodies.append(np.asarray(row, F))
        self.types.append(kind)
        return len(self.bodies) - 1

    # -- constraints -----------------------------------------------------------
    def add_contact(self, ref, alt, normal, points, lam=0.0):
        row = np.zeros(CONTACT_STRIDE, F)
        row[0:3] = normal
        pts = np.asarray(points, F).reshape(-1, 4)
        assert 1 <= len(pts) <= 4 and ref != alt
        row[3:3 + 4 * len(pts)] = pts.reshape(-1)
        self.contacts.append(row)
        self.cints.append((ref, alt, len(pts)))
        self.lambdas.append(lam)

    def add_fixed(self, b1, b2, r1, r2, attach1, attach2, separation):
        row = np.zeros(JOINT_STRIDE, F)
        row[0:3], row[3:6] = r1, r2
        row[6:10], row[10:14], row[14] = attach1, attach2, separation
        self.joints.append(row)
        self.jints.append((FIXED, b1, b2))

    def add_hinge(self, b1, b2, r1, r2, a1, a2):
        row = np.zeros(JOINT_STRIDE, F)
        row[0:3], row[3:6] = r1, r2
        row[6:9], row[9:12] = a1, a2
        self.joints.append(row)
        self.jints.append((HINGE, b1, b2))

    # -- frozen arrays ---------------------------------------------------------
    def freeze(self):
        self.bodies = np.ascontiguousarray(
            np.array(self.bodies, F).reshape(-1, BODY_STRIDE))
        self.types = np.array(self.types, np.int32)
        self.contacts = np.ascontiguousarray(
            np.array(self.contacts, F).reshape(-1, CONTACT_STRIDE))
        self.cints = np.array(self.cints, np.int32).reshape(-1, 3)
        self.joints = np.ascontiguousarray(
            np.array(self.joints, F).reshape(-1, JOINT_STRIDE))
        self.jints = np.array(self.jints, np.int32).reshape(-1, 3)
        self.lambdas = np.array(self.lambdas, F)
        return self

    def inv_mass(self, b):
        """The inverse mass the solver uses (Static bodies: 0)."""
        return 0.0 if self.types[b] == STATIC else float(self.bodies[b][33])


# ------------------------------------------------------------------------------
# pieces
# ------------------------------------------------------------------------------
def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def rand_unit(rng):
    return unit(rng.normal(size=3))


def rand_quat(rng, tilt):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(-tilt, tilt)
    return np.concatenate([[np.cos(angle / 2)],
                           np.sin(angle / 2) * axis]).astype(F)


IDENTITY = np.array([1, 0, 0, 0], F)


def body_row(rng, pos=None, rot=None, moving=True, inv_mass=None,
             inv_inertia=None, at_rest_pose=False, forces=False):
    """A near-resting body.  at_rest_pose: previous = pre-solve = current pose
    (nothing has moved it yet this substep)."""
    row = np.zeros(BODY_STRIDE, F)
    pos = rng.uniform(-2, 2, 3) if pos is None else pos
    rot = rand_quat(rng, 0.2) if rot is None else rot
    row[0:3], row[3:7] = pos, rot
    if moving:
        row[7:10] = rng.uniform(-0.5, 0.5, 3)
        row[10:13] = rng.uniform(-0.3, 0.3, 3)
    if at_rest_pose:
        row[13:16], row[16:20] = row[0:3], row[3:7]
        row[20:23], row[23:27] = row[0:3], row[3:7]
    else:
        # previous pose a substep back along the velocity; the pre-solve pose
        # is the current one, or a hair off it (an earlier constraint moved it)
        row[13:16] = row[0:3] - H * row[7:10] + rng.uniform(-1e-4, 1e-4, 3).astype(F)
        row[16:20] = unit(row[3:7] + rng.uniform(-2e-3, 2e-3, 4))
        row[20:23], row[23:27] = row[0:3], row[3:7]
        if rng.random() < 0.5:
            row[20:23] += rng.uniform(-1e-3, 1e-3, 3).astype(F)
            row[23:27] = unit(row[3:7] + rng.uniform(-1e-3, 1e-3, 4))
    row[27:30] = row[7:10] + rng.uniform(-0.05, 0.05, 3).astype(F) * moving
    row[30:33] = row[10:13] + rng.uniform(-0.05, 0.05, 3).astype(F) * moving
    row[33] = rng.uniform(0.2, 2.0) if inv_mass is None else inv_mass
    row[34:37] = rng.uniform(0.5, 5.0, 3) if inv_inertia is None else inv_inertia
    row[37] = rng.uniform(0.3, 1.0)
    row[38] = rng.uniform(0.2, 0.8)
    if forces:
        row[39:42] = rng.uniform(-2, 2, 3)
        row[42:45] = rng.uniform(-1, 1, 3)
    return row


def static_row(rng, rot=IDENTITY, pos=None):
    # the metadata keeps a non-zero mass: the solver must zero it for Static
    return body_row(rng, pos=pos, rot=np.asarray(rot, F), moving=False,
                    at_rest_pose=True)


def contact_points(rng, w, ref, n_pts, depths=None):
    """n_pts points round the reference body with the given depths."""
    centre = w.bodies[ref][0:3]
    depths = rng.uniform(0.002, 0.03, n_pts) if depths is None else depths
    pts = [np.concatenate([centre + rng.uniform(-0.5, 0.5, 3), [d]])
           for d in depths]
    return np.array(pts, F)


def random_contact(rng, w, ref, alt, n_pts=None, depths=None, normal=None,
                   lam=None):
    n_pts = int(rng.integers(1, 5)) if n_pts is None else n_pts
    normal = rand_unit(rng) if normal is None else normal
    lam = -rng.uniform(0, 0.02) if lam is None else lam
    w.add_contact(ref, alt, normal, contact_points(rng, w, ref, n_pts, depths),
                  lam)


# ------------------------------------------------------------------------------
# family 1: contact pairs
# ------------------------------------------------------------------------------
# a rotation that normalize() moves: the length is off by a part in a thousand
def not_normalised(rng):
    return (rand_quat(rng, 0.4).astype(np.float64) * 1.001).astype(F)


def family_contact_pairs(n=128, seed=101):
    rng = np.random.default_rng(seed)
    kinds = ["dyn_dyn", "dyn_static", "static_dyn", "static_inert_flip",
             "static_tilted", "static_not_normalised", "static_neg_zero",
             "inertia_1", "inertia_2", "inertia_3", "unequal_mass",
             "kinematic"]
    worlds = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        w = World("pairs/" + kind)
        a = w.add_body(body_row(rng))
        if kind == "dyn_dyn":
            b = w.add_body(body_row(rng))
        elif kind in ("dyn_static", "static_dyn"):
            b = w.add_body(static_row(rng), STATIC)
        elif kind == "static_inert_flip":
            flip = np.roll(IDENTITY, 1 + i % 3)     # half turn about x / y / z
            b = w.add_body(static_row(rng, flip), STATIC)
        elif kind == "static_tilted":
            b = w.add_body(static_row(rng, rand_quat(rng, 0.6)), STATIC)
        elif kind == "static_not_normalised":
            b = w.add_body(static_row(rng, not_normalised(rng)), STATIC)
        elif kind == "static_neg_zero":
            pos = rng.uniform(-1, 1, 3).astype(F)
            pos[rng.integers(0, 3)] = F(-0.0)
            pos[rng.integers(0, 3)] = F(-0.0)
            row = static_row(rng, pos=pos)
            assert np.signbit(row[0:3]).any() and np.signbit(row[13:16]).any()
            b = w.add_body(row, STATIC)
        elif kind.startswith("inertia_"):
            inv_i = rng.uniform(0.5, 5.0, 3)
            inv_i[rng.permutation(3)[:int(kind[-1])]] = 0.0
            b = w.add_body(body_row(rng, inv_inertia=inv_i))
        elif kind == "unequal_mass":
            b = w.add_body(body_row(rng, inv_mass=rng.choice([1e-4, 2e3])))
        else:
            b = w.add_body(body_row(rng), KINEMATIC)
        # (either body as the reference one, in every kind)
        swap = {"dyn_static": False, "static_dyn": True}.get(
            kind, (i // len(kinds)) % 2 == 1)
        ref, alt = (b, a) if swap else (a, b)
        for _ in range(1 + i % 3):
            random_contact(rng, w, ref, alt)
        worlds.append(w.freeze())
    return worlds


# ------------------------------------------------------------------------------
# family 2: contact geometry
# ------------------------------------------------------------------------------
def _resting_pair(rng, w, other_static):
    """Two bodies nothing has moved yet: identity rotations, previous and
    pre-solve pose equal to the current one."""
    a = w.add_body(body_row(rng, rot=IDENTITY, at_rest_pose=True))
    if other_static:
        b = w.add_body(static_row(rng), STATIC)
    else:
        b = w.add_body(body_row(rng, rot=IDENTITY, at_rest_pose=True))
    return a, b


def family_contact_geometry(n=128, seed=202):
    rng = np.random.default_rng(seed)
    kinds = ["points_1", "points_2", "points_3", "points_4", "separated_pose",
             "negative_depths", "barely", "deep", "zero_depths",
             "cancelling_depths", "no_tangent", "stick", "slide"]
    worlds = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        w = World("geometry/" + kind)
        if kind.startswith("points_"):
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            random_contact(rng, w, a, b, n_pts=int(kind[-1]))
        elif kind == "separated_pose":
            # the reference body has since moved back along the normal by more
            # than the depth: d <= 0, lambda_n stays 0
            normal = rand_unit(rng)
            row = body_row(rng)
            row[20:23], row[23:27] = row[0:3], row[3:7]
            row[0:3] -= F(0.1) * normal
            a, b = w.add_body(row), w.add_body(body_row(rng))
            random_contact(rng, w, a, b, normal=normal)
        elif kind == "negative_depths":
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            n_pts = int(rng.integers(1, 5))
            random_contact(rng, w, a, b, n_pts=n_pts,
                           depths=-rng.uniform(0.01, 0.03, n_pts))
        elif kind == "barely":
            a, b = _resting_pair(rng, w, i % 2 == 0)
            n_pts = int(rng.integers(1, 5))
            random_contact(rng, w, a, b, n_pts=n_pts,
                           depths=rng.uniform(1e-7, 1e-6, n_pts))
        elif kind == "deep":
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            n_pts = int(rng.integers(1, 5))
            random_contact(rng, w, a, b, n_pts=n_pts,
                           depths=rng.uniform(0.3, 1.0, n_pts))
        elif kind == "zero_depths":
            # getAvgContact: penetration_sum == 0 -> zero separation
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            n_pts = int(rng.integers(1, 5))
            random_contact(rng, w, a, b, n_pts=n_pts, depths=np.zeros(n_pts))
        elif kind == "cancelling_depths":
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            d = F(rng.uniform(0.01, 0.03))
            random_contact(rng, w, a, b, n_pts=2, depths=[d, -d])
        elif kind == "no_tangent":
            # axis-aligned normal through both centres, identity rotations,
            # nothing moved yet: no torque arm, the correction is along the
            # normal only and the tangential displacement is exactly 0
            a, b = _resting_pair(rng, w, i % 2 == 0)
            axis = i % 3
            pos_b = w.bodies[a][0:3].copy()
            pos_b[axis] -= F(1.0)
            for s in (0, 13, 20):
                w.bodies[b][s:s + 3] = pos_b
            normal = np.zeros(3, F)
            normal[axis] = 1
            pt = w.bodies[a][0:3].copy()
            pt[axis] -= F(0.5)
            w.add_contact(a, b, normal, [[*pt, rng.uniform(0.005, 0.02)]],
                          -0.01)
        else:
            # the reference body has slid sideways since the previous pose, by
            # little (static friction holds: lambda_t > lambda_n * mu_s) or by
            # a lot (it does not)
            a, b = _resting_pair(rng, w, i % 2 == 0)
            normal = np.array([0, 0, 1], F)
            slip = 1e-5 if kind == "stick" else 0.05
            w.bodies[a][13:16] -= np.array([slip, 0.5 * slip, 0], F)
            random_contact(rng, w, a, b, normal=normal,
                           depths=rng.uniform(0.01, 0.02, 2), n_pts=2)
        worlds.append(w.freeze())
    return worlds


# ------------------------------------------------------------------------------
# family 3: velocity solve
# ------------------------------------------------------------------------------
def family_velocity(n=128, seed=303):
    rng = np.random.default_rng(seed)
    kinds = ["below", "at", "above", "no_tangential_velocity", "zero_lambda",
             "unequal_depths"]
    worlds = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        w = World("velocity/" + kind)
        if kind in ("below", "at", "above", "no_tangential_velocity"):
            # pre-solve velocity along an axis-aligned normal with no spin: v_bar
            # is that velocity itself and vn_bar one of its components
            a, b = _resting_pair(rng, w, i % 2 == 0)
            axis = i % 3
            normal = np.zeros(3, F)
            normal[axis] = 1
            speed = {"below": np.nextafter(THRESHOLD, F(0)),
                     "at": THRESHOLD,
                     "above": np.nextafter(THRESHOLD, F(1)),
                     "no_tangential_velocity": F(4) * THRESHOLD}[kind]
            for row in (w.bodies[a], w.bodies[b]):
                row[7:13] = 0
                row[27:33] = 0
            # (fminf(-e * vn_bar, 0): the coefficient only shows for vn_bar > 0)
            w.bodies[a][27 + axis] = speed
            w.bodies[a][7 + axis] = speed * F(0.5)
            if kind == "no_tangential_velocity":
                # contact point on the axis through the reference body's
                # centre: no tangential component anywhere
                pt = w.bodies[a][0:3].copy()
                w.add_contact(a, b, normal, [[*pt, 0.01]], -0.02)
            else:
                w.bodies[a][7 + (axis + 1) % 3] = F(rng.uniform(-0.3, 0.3))
                random_contact(rng, w, a, b, normal=normal)
        elif kind == "zero_lambda":
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            n_pts = int(rng.integers(1, 5))
            # (negative depths: the position solve leaves lambda_n at 0 too)
            random_contact(rng, w, a, b, n_pts=n_pts, lam=0.0,
                           depths=-rng.uniform(0.01, 0.03, n_pts))
        else:
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            n_pts = int(rng.integers(2, 5))
            depths = rng.uniform(0.001, 0.002, n_pts)
            depths[0] = rng.uniform(0.05, 0.2)
            random_contact(rng, w, a, b, n_pts=n_pts, depths=depths)
        worlds.append(w.freeze())
    return worlds


# ------------------------------------------------------------------------------
# family 4: joints
# ------------------------------------------------------------------------------
def _joint_anchor(rng):
    return rng.uniform(-0.5, 0.5, 3).astype(F)


def _random_joint(rng, w, b1, b2):
    if rng.random() < 0.5:
        w.add_fixed(b1, b2, _joint_anchor(rng), _joint_anchor(rng),
                    rand_quat(rng, 0.5), rand_quat(rng, 0.5),
                    rng.uniform(0, 0.5))
    else:
        w.add_hinge(b1, b2, _joint_anchor(rng), _joint_anchor(rng),
                    rand_unit(rng), rand_unit(rng))


def family_joints(n=128, seed=404):
    rng = np.random.default_rng(seed)
    kinds = ["fixed_aligned", "fixed_satisfied", "fixed_separation",
             "fixed_static", "hinge_static", "hinge_parallel",
             "hinge_antiparallel", "chain", "same_pair", "count_1", "count_2",
             "count_3", "max_bodies"]
    worlds = []
    for i in range(n):
        kind = kinds[i % len(kinds)]
        w = World("joints/" + kind)
        if kind == "fixed_aligned":
            # same rotation, same attach rotation: diff is q q^-1, delta_q 0
            rot = IDENTITY if i % 2 else np.array([0, 1, 0, 0], F)
            a = w.add_body(body_row(rng, rot=rot))
            b = w.add_body(body_row(rng, rot=rot))
            w.add_fixed(a, b, _joint_anchor(rng), _joint_anchor(rng),
                        IDENTITY, IDENTITY, rng.uniform(0, 0.5))
        elif kind == "fixed_satisfied":
            # identity everything, both anchors at the same world point and no
            # separation: delta_q and pos_correction are exactly 0
            pos = rng.integers(-8, 8, 3).astype(F) * F(0.25)
            r = rng.integers(-4, 4, 3).astype(F) * F(0.125)
            a = w.add_body(body_row(rng, pos=pos, rot=IDENTITY))
            b = w.add_body(body_row(rng, pos=pos + r, rot=IDENTITY))
            w.add_fixed(a, b, r, np.zeros(3, F), IDENTITY, IDENTITY, 0.0)
        elif kind == "fixed_separation":
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            w.add_fixed(a, b, _joint_anchor(rng), _joint_anchor(rng),
                        rand_quat(rng, 0.5), rand_quat(rng, 0.5),
                        rng.uniform(0.5, 2.0))
        elif kind in ("fixed_static", "hinge_static"):
            a = w.add_body(body_row(rng))
            b = w.add_body(static_row(rng, rand_quat(rng, 0.5) if i % 2
                                      else IDENTITY), STATIC)
            b1, b2 = (a, b) if (i // 2) % 2 else (b, a)
            if kind == "fixed_static":
                w.add_fixed(b1, b2, _joint_anchor(rng), _joint_anchor(rng),
                            rand_quat(rng, 0.5), rand_quat(rng, 0.5),
                            rng.uniform(0, 0.5))
            else:
                w.add_hinge(b1, b2, _joint_anchor(rng), _joint_anchor(rng),
                            rand_unit(rng), rand_unit(rng))
        elif kind in ("hinge_parallel", "hinge_antiparallel"):
            # identity rotations and one axis-aligned axis: the cross product
            # of the two world axes is exactly 0
            a = w.add_body(body_row(rng, rot=IDENTITY))
            b = w.add_body(body_row(rng, rot=IDENTITY))
            axis = np.zeros(3, F)
            axis[i % 3] = 1
            w.add_hinge(a, b, _joint_anchor(rng), _joint_anchor(rng), axis,
                        axis if kind == "hinge_parallel" else -axis)
        elif kind == "chain":
            count = 3 + i % 6       # 3..8 joints, each sharing a body with the next
            ids = [w.add_body(body_row(rng)) for _ in range(count + 1)]
            for k in range(count):
                _random_joint(rng, w, ids[k], ids[k + 1])
        elif kind == "same_pair":
            a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
            _random_joint(rng, w, a, b)
            _random_joint(rng, w, b, a)
        elif kind.startswith("count_"):
            # disjoint pairs; 3 is the first count whose row lies in HBM
            for _ in range(int(kind[-1])):
                _random_joint(rng, w, w.add_body(body_row(rng)),
                              w.add_body(body_row(rng)))
        else:
            # as many joints as a world can hold, over as many bodies
            ids = [w.add_body(body_row(rng)) for _ in range(16)]
            for k in range(8):
                _random_joint(rng, w, ids[2 * k], ids[2 * k + 1])
        worlds.append(w.freeze())
    return worlds


# ------------------------------------------------------------------------------
# family 5: level structure
# ------------------------------------------------------------------------------
def level_world(rng, lpw, kind, max_bodies=MAX_BODIES):
    """One world of the level-structure family."""
    w = World("levels/%s/%d" % (kind, lpw))
    if kind in ("none", "one"):
        a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
        if kind == "one":
            random_contact(rng, w, a, b)
    elif kind == "chain":
        # every contact shares body 0: levels 0 .. n - 1
        hub = w.add_body(body_row(rng, inv_mass=0.3))
        for _ in range(12):
            random_contact(rng, w, hub, w.add_body(body_row(rng)))
    elif kind in ("star_inert", "star_tilted"):
        # lpw / 2 + 3 contacts round one static body, each with a dynamic body
        # of its own: round an inert floor they all land at level 0 (more than
        # lpw / 2 teams: a second round); round a floor that normalize() moves
        # they serialise.  (Contacts of one level share no body, so this is the
        # one kind that needs more than MAX_BODIES bodies at 64 lanes: 36.)
        count = lpw // 2 + 3
        rot = IDENTITY if kind == "star_inert" else not_normalised(rng)
        floor = w.add_body(static_row(rng, rot), STATIC)
        for k in range(count):
            body = w.add_body(body_row(rng), limit=count + 1)
            if k % 2:
                random_contact(rng, w, body, floor)
            else:
                random_contact(rng, w, floor, body)
    elif kind in ("lpw", "lpw_plus_1", "two_lpw_plus_3"):
        count = {"lpw": lpw, "lpw_plus_1": lpw + 1,
                 "two_lpw_plus_3": 2 * lpw + 3}[kind]
        floor = w.add_body(static_row(rng), STATIC)
        ids = [w.add_body(body_row(rng)) for _ in range(max_bodies - 1)]
        for k in range(count):
            # random pairs over few bodies: deep, irregular level structure,
            # with the floor mixed in
            a, b = rng.choice(ids, 2, replace=False)
            if rng.random() < 0.25:
                b = floor
            if rng.random() < 0.5:
                a, b = b, a
            random_contact(rng, w, int(a), int(b), n_pts=1 + k % 4,
                           depths=rng.uniform(0.001, 0.004, 1 + k % 4))
    else:
        assert kind == "contact_and_joint"
        a, b = w.add_body(body_row(rng)), w.add_body(body_row(rng))
        random_contact(rng, w, a, b)
        _random_joint(rng, w, b, a)
    return w.freeze()


LEVEL_KINDS = ("none", "one", "chain", "star_inert", "star_tilted", "lpw",
               "lpw_plus_1", "two_lpw_plus_3", "contact_and_joint")


def family_levels(lpw, max_contacts=None, max_bodies=MAX_BODIES, n=128,
                  seed=505):
    """max_contacts, max_bodies: the caps of the instantiation under test (None:
    no cap on the contacts); kinds that need more contacts are left out."""
    rng = np.random.default_rng(seed + lpw)
    kinds = [k for k in LEVEL_KINDS
             if max_contacts is None or
             {"lpw_plus_1": lpw + 1, "two_lpw_plus_3": 2 * lpw + 3}.get(k, 0)
             <= max_contacts]
    return [level_world(rng, lpw, kinds[i % len(kinds)], max_bodies)
            for i in range(n)]


# ------------------------------------------------------------------------------
# family 6: asymmetric halves (neighbouring worlds share a wavefront)
# ------------------------------------------------------------------------------
def family_asymmetric(lpw=32, max_bodies=MAX_BODIES, n=128, seed=606):
    rng = np.random.default_rng(seed)
    pairs = [("none", "lpw"), ("one", "chain"), ("contact_and_joint", "one"),
             ("lpw", "none"), ("chain", "star_inert")]
    worlds = []
    for i in range(n // 2):
        left, right = pairs[i % len(pairs)]
        if left == "contact_and_joint" and i % 2:
            # joints beside none: a joint chain next to a world without any
            w = World("asymmetric/joint_chain")
            ids = [w.add_body(body_row(rng)) for _ in range(5)]
            for k in range(4):
                _random_joint(rng, w, ids[k], ids[k + 1])
            worlds.append(w.freeze())
        else:
            worlds.append(level_world(rng, lpw, left, max_bodies))
        worlds.append(level_world(rng, lpw, right, max_bodies))
    for w in worlds:
        w.tag = "asymmetric/" + w.tag
    return worlds


# ------------------------------------------------------------------------------
# family 7: random worlds
# ------------------------------------------------------------------------------
def family_random(n=192, seed=707, max_contacts=40, max_bodies=MAX_BODIES):
    rng = np.random.default_rng(seed)
    worlds = []
    for i in range(n):
        w = World("random")
        nb = int(rng.integers(2, max_bodies + 1))
        for k in range(nb):
            if rng.random() < 0.2:
                rot = IDENTITY if rng.random() < 0.5 else rand_quat(rng, 0.5)
                w.add_body(static_row(rng, rot), STATIC)
            else:
                w.add_body(body_row(rng, forces=rng.random() < 0.3),
                           KINEMATIC if rng.random() < 0.1 else DYNAMIC)
        if all(t == STATIC for t in w.types):
            w.types[0] = DYNAMIC

        def pair():
            while True:
                a, b = rng.choice(nb, 2, replace=False)
                if w.types[a] != STATIC or w.types[b] != STATIC:
                    return int(a), int(b)

        for _ in range(int(rng.integers(0, max_contacts + 1))):
            random_contact(rng, w, *pair())
        for _ in range(int(rng.integers(0, 9))):
            _random_joint(rng, w, *pair())
        worlds.append(w.freeze())
    return worlds


def all_families(lpw=64, max_contacts=None, max_bodies=MAX_BODIES):
    """Every family, within what the instantiation under test can hold: lpw lanes
    per world, at most max_contacts contacts (None: no cap) and max_bodies
    bodies the solver can change."""
    return {
        "pairs": family_contact_pairs(),
        "geometry": family_contact_geometry(),
        "velocity": family_velocity(),
        "joints": family_joints(),
        "levels": family_levels(lpw, max_contacts, max_bodies),
        "asymmetric": family_asymmetric(min(lpw, 32), max_bodies),
        "random": family_random(
            max_contacts=40 if max_contacts is None else min(40, max_contacts),
            max_bodies=max_bodies),
    }


# ------------------------------------------------------------------------------
# the greedy level rule (phys_impl/step_hbm.inl constraintLevels)
# ------------------------------------------------------------------------------
def greedy_levels(keys_a, keys_b):
    """Level of constraint i: 1 + the highest level of any earlier constraint
    that shares a non-zero key with it, 0 when there is none.  Key 0 (an inert
    static body, or no body) never conflicts."""
    levels = []
    for i, (a, b) in enumerate(zip(keys_a, keys_b)):
        level = 0
        for j in range(i):
            ja, jb = keys_a[j], keys_b[j]
            conflict = (ja != 0 and ja in (a, b)) or (jb != 0 and jb in (a, b))
            if conflict and levels[j] + 1 > level:
                level = levels[j] + 1
        levels.append(level)
    return levels


# ------------------------------------------------------------------------------
# running a C solve_world entry point
# ------------------------------------------------------------------------------
def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


SOLVE_ARGS = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32,
              C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32,
              C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32,
              C.POINTER(C.c_float), C.c_uint32,
              C.POINTER(C.c_float), C.POINTER(C.c_float)]


def bind_solve(fn):
    fn.restype = C.c_int32
    fn.argtypes = SOLVE_ARGS
    return fn


def solve(fn, w, mask):
    """(body state [nb, 33], lambdas [nc]) after the phases in `mask`."""
    out = np.zeros((len(w.bodies), BODY_STATE), F)
    lambdas = w.lambdas.copy()
    # (ctypes needs a buffer even when there is nothing in it)
    pad = np.zeros(1, F)
    rc = fn(_ptr(w.bodies, C.c_float), _ptr(w.types, C.c_int32), len(w.bodies),
            _ptr(w.contacts if len(w.contacts) else pad, C.c_float),
            _ptr(w.cints, C.c_int32), len(w.contacts),
            _ptr(w.joints if len(w.joints) else pad, C.c_float),
            _ptr(w.jints, C.c_int32), len(w.joints),
            _ptr(w.sys, C.c_float), mask,
            _ptr(out, C.c_float), _ptr(lambdas if len(lambdas) else pad,
                                       C.c_float))
    assert rc == 0, (w.tag, rc)
    return out, lambdas


def check_input_conditions(w):
    """Holds for the reference alone: no constraint joins two bodies that both
    have zero inverse mass (it would divide by w1 + w2 = 0)."""
    for a, b, _ in w.cints:
        assert w.inv_mass(a) != 0 or w.inv_mass(b) != 0, w.tag
    for _, a, b in w.jints:
        assert w.inv_mass(a) != 0 or w.inv_mass(b) != 0, w.tag


# ------------------------------------------------------------------------------
# many worlds in one call (tests/shims/phys_device_shim.hip dev_solve_worlds)
# ------------------------------------------------------------------------------
DEV_SOLVE_ARGS = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                  C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                  C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                  C.POINTER(C.c_float), C.c_uint32, C.c_int32, C.c_int32,
                  C.POINTER(C.c_float), C.POINTER(C.c_float),
                  C.POINTER(C.c_int32)]


def bind_dev_solve(fn):
    fn.restype = C.c_int32
    fn.argtypes = DEV_SOLVE_ARGS
    return fn


class Packed:
    """Worlds laid end to end, with the offsets of each."""

    def __init__(self, worlds):
        def cat(rows, width, dtype):
            rows = [r.reshape(-1, width) for r in rows]
            return np.ascontiguousarray(
                np.concatenate(rows + [np.zeros((1, width), dtype)]), dtype)

        def offsets(counts):
            return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

        self.worlds = worlds
        self.bodies = cat([w.bodies for w in worlds], BODY_STRIDE, F)
        self.types = cat([w.types for w in worlds], 1, np.int32)
        self.contacts = cat([w.contacts for w in worlds], CONTACT_STRIDE, F)
        self.cints = cat([w.cints for w in worlds], 3, np.int32)
        self.joints = cat([w.joints for w in worlds], JOINT_STRIDE, F)
        self.jints = cat([w.jints for w in worlds], 3, np.int32)
        self.lambdas = cat([w.lambdas for w in worlds], 1, F)
        self.sys = cat([w.sys for w in worlds], 5, F)
        self.body_off = offsets([len(w.bodies) for w in worlds])
        self.contact_off = offsets([len(w.contacts) for w in worlds])
        self.joint_off = offsets([len(w.joints) for w in worlds])


def dev_solve(fn, packed, mask, mode):
    """[(body state, lambdas)] per world after the phases in `mask`."""
    p = packed
    out = np.zeros((len(p.bodies), BODY_STATE), F)
    lambdas = p.lambdas.copy()
    status = np.full(len(p.worlds), -99, np.int32)
    rc = fn(_ptr(p.bodies, C.c_float), _ptr(p.types, C.c_int32),
            _ptr(p.body_off, C.c_int32),
            _ptr(p.contacts, C.c_float), _ptr(p.cints, C.c_int32),
            _ptr(p.contact_off, C.c_int32),
            _ptr(p.joints, C.c_float), _ptr(p.jints, C.c_int32),
            _ptr(p.joint_off, C.c_int32),
            _ptr(p.sys, C.c_float), mask, len(p.worlds), mode,
            _ptr(out, C.c_float), _ptr(lambdas, C.c_float),
            _ptr(status, C.c_int32))
    assert rc == 0, rc
    assert (status == 0).all(), [(w.tag, int(s)) for w, s in
                                 zip(p.worlds, status) if s != 0][:8]
    lambdas = lambdas.reshape(-1)
    return [(out[p.body_off[i]:p.body_off[i + 1]],
             lambdas[p.contact_off[i]:p.contact_off[i + 1]])
            for i in range(len(p.worlds))]
