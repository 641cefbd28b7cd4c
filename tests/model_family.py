"""A family of generated MJCF models that stand on the edges of what csrc/mjcf_loader.cpp compiles for the run-time-topology
instantiations of the step kernel (launch_step<32, TopoRuntime>, launch_step<40, TopoRuntime>), and a sampler of states for them --
test infrastructure only.

generate(member, directory, seed) is a pure function of (member, seed): it writes <directory>/<member>.xml and returns the path.
Every model has a ground plane, bodies with an explicit <inertial> (inertiafromgeom="false": masses 0.3 .. 2 kg, principal inertias
2e-3 .. 2e-2 that obey the triangle inequality, a random inertial frame), joints with random unit axes, anchors off the body's origin,
random damping, a mix of zero and non-zero armature / stiffness / springref, ranges on about half of the hinges and slides, and sphere
/ capsule / box geoms on a chosen subset of the bodies: class "all" geoms collide with everything, class "floor" geoms with the plane
only, so the candidate pairs stay far below CM_MAXPAIR.

MEMBERS is the table of the members (what is exact about each is asserted on the loaded pod by tests/test_model_family.py), REFUSALS
the table of one-off models the loader must refuse, each with the message it must give."""
import os
import zlib

import numpy as np

# ------------------------------------------------------------------------------------------------------------ the builder


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def _fmt(v):
    return " ".join(repr(float(x)) for x in np.atleast_1d(v))


class _Builder:
    def __init__(self, name, seed):
        self.name = name
        self.rng = np.random.default_rng([int(seed), zlib.crc32(name.encode())])
        self.bodies, self.equalities, self.motors, self.sensors = [], [], [], []

    # -- random parts
    def _quat(self, tilt=None):
        """A random unit quaternion: anywhere on the sphere, or (tilt) a turn about z times a tilt of at most `tilt` rad."""
        r = self.rng
        if tilt is None:
            return _unit(r.standard_normal(4))
        a, t = r.uniform(-np.pi, np.pi), r.uniform(0, tilt)
        ax = _unit([r.standard_normal(), r.standard_normal(), 0.0])
        qz = np.array([np.cos(a / 2), 0, 0, np.sin(a / 2)])
        qt = np.concatenate([[np.cos(t / 2)], np.sin(t / 2) * ax])
        w1, x1, y1, z1 = qz
        w2, x2, y2, z2 = qt
        return _unit([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                      w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])

    def _joint(self, kind, limited=None, axis=None):
        r = self.rng
        j = dict(type=kind, damping=r.uniform(0.05, 0.5), armature=0.0, stiffness=0.0, springref=0.0, limited=False, range=(0.0, 0.0),
                 axis=_unit(r.standard_normal(3)) if axis is None else _unit(axis), pos=np.zeros(3))
        if r.random() < 0.5:
            j["armature"] = r.uniform(0.005, 0.05)
        if kind == "free":
            j["damping"] = r.uniform(0.0, 0.1)
            return j
        j["pos"] = r.uniform(-0.02, 0.02, 3)                    # the anchor sits off the body's origin
        if kind in ("hinge", "slide"):
            if r.random() < 0.5:
                j["stiffness"] = r.uniform(1.0, 10.0)
            if r.random() < 0.5:
                j["springref"] = r.uniform(-0.3, 0.3) * (1.0 if kind == "hinge" else 0.2)
            if (r.random() < 0.5) if limited is None else limited:
                s = 1.0 if kind == "hinge" else 0.12
                j["limited"], j["range"] = True, (-r.uniform(0.3, 1.2) * s, r.uniform(0.3, 1.2) * s)
        return j

    def _geom(self, spec):
        kind, cls = spec
        r = self.rng
        size = {"sphere": [r.uniform(0.03, 0.034)], "capsule": [r.uniform(0.03, 0.034), r.uniform(0.01, 0.02)],
                "box": list(r.uniform(0.03, 0.034, 3))}[kind]
        return dict(type=kind, cls=cls, size=size, pos=r.uniform(-0.01, 0.01, 3) * [1, 1, 0.3],
                    quat=self._quat(tilt=0.05 if kind == "box" else None), friction=r.uniform(0.6, 1.2))

    def body(self, parent, joints=(), geom=None, pos=(0.07, 0.0, 0.0), site=False, limited=None, axes=None):
        """Adds a body under `parent` (-1: the world); joints: a sequence of "hinge" / "slide" / "ball" / "free"; geom: None or
        (type, "all" | "floor"); -> its index."""
        r = self.rng
        sq = r.uniform(1e-3, 1e-2, 3)                            # a box's x^2, y^2, z^2: its principal inertias obey the triangle inequality
        b = dict(parent=parent, pos=np.asarray(pos, dtype=np.float64), quat=self._quat(tilt=0.05), mass=r.uniform(0.3, 2.0),
                 ipos=r.uniform(-0.02, 0.02, 3), iquat=self._quat(), inertia=np.array([sq[1] + sq[2], sq[0] + sq[2], sq[0] + sq[1]]),
                 joints=[self._joint(k, limited, None if axes is None else axes[i]) for i, k in enumerate(joints)],
                 geom=None if geom is None else self._geom(geom), site=None)
        if site:
            b["site"] = dict(pos=r.uniform(-0.03, 0.03, 3), quat=self._quat())
        self.bodies.append(b)
        return len(self.bodies) - 1

    def chain(self, parent, n, joints=("hinge",), geom_every=0, step=(0.07, 0.0, 0.0), geom=("sphere", "floor"), first_pos=None, site_every=0):
        """n bodies in a line under `parent`, each with `joints`; -> the index of the last."""
        for k in range(n):
            parent = self.body(parent, joints, geom if geom_every and k % geom_every == 0 else None,
                               pos=first_pos if (k == 0 and first_pos is not None) else step, site=bool(site_every) and k % site_every == 0)
        return parent

    def joint_name(self, b, k=0):
        return "j%d_%d" % (b, k)

    # -- the text
    def xml(self):
        out = ['<mujoco model="%s">' % self.name,
               '  <compiler angle="radian" inertiafromgeom="false"/>',
               '  <option timestep="0.0005" iterations="50" solver="PGS" magnetic="0 -0.5 0.3"/>',
               '  <worldbody>',
               '    <geom name="floor" type="plane" size="5 5 0.1" contype="1" conaffinity="3"/>']
        kids = {}
        for i, b in enumerate(self.bodies):
            kids.setdefault(b["parent"], []).append(i)

        def emit(i, ind):
            b = self.bodies[i]
            out.append('%s<body name="b%d" pos="%s" quat="%s">' % (ind, i, _fmt(b["pos"]), _fmt(b["quat"])))
            out.append('%s  <inertial pos="%s" quat="%s" mass="%s" diaginertia="%s"/>' % (ind, _fmt(b["ipos"]), _fmt(b["iquat"]), _fmt(b["mass"]), _fmt(b["inertia"])))
            for k, j in enumerate(b["joints"]):
                a = 'name="%s" type="%s" damping="%s" armature="%s"' % (self.joint_name(i, k), j["type"], _fmt(j["damping"]), _fmt(j["armature"]))
                if j["type"] != "free":
                    a += ' pos="%s"' % _fmt(j["pos"])
                if j["type"] in ("hinge", "slide"):
                    a += ' axis="%s" stiffness="%s" springref="%s"' % (_fmt(j["axis"]), _fmt(j["stiffness"]), _fmt(j["springref"]))
                    if j["limited"]:
                        a += ' limited="true" range="%s"' % _fmt(j["range"])
                out.append('%s  <joint %s/>' % (ind, a))
            g = b["geom"]
            if g is not None:
                ct, ca = (1, 1) if g["cls"] == "all" else (2, 0)
                out.append('%s  <geom name="g%d" type="%s" size="%s" pos="%s" quat="%s" contype="%d" conaffinity="%d" friction="%s 0.005 0.0001"/>'
                           % (ind, i, g["type"], _fmt(g["size"]), _fmt(g["pos"]), _fmt(g["quat"]), ct, ca, _fmt(g["friction"])))
            if b["site"] is not None:
                out.append('%s  <site name="s%d" pos="%s" quat="%s"/>' % (ind, i, _fmt(b["site"]["pos"]), _fmt(b["site"]["quat"])))
            for c in kids.get(i, []):
                emit(c, ind + "  ")
            out.append('%s</body>' % ind)

        for i in kids.get(-1, []):
            emit(i, "    ")
        out.append('  </worldbody>')
        if self.equalities:
            out.append('  <equality>')
            for b1, b2, anchor in self.equalities:
                out.append('    <connect body1="b%d" body2="b%d" anchor="%s" solref="0.005 1"/>' % (b1, b2, _fmt(anchor)))
            out.append('  </equality>')
        if self.motors:
            out.append('  <actuator>')
            for k, (joint, gear, hi) in enumerate(self.motors):
                out.append('    <motor name="m%d" joint="%s" gear="%s" ctrllimited="true" ctrlrange="%s %s"/>' % (k, joint, _fmt(gear), _fmt(-hi), _fmt(hi)))
            out.append('  </actuator>')
        if self.sensors:
            out.append('  <sensor>')
            out.extend('    ' + s for s in self.sensors)
            out.append('  </sensor>')
        out.append('</mujoco>')
        return "\n".join(out) + "\n"


# ------------------------------------------------------------------------------------------------------------ the members
ROOT_Z = 0.03      # where a tree hung on the world (no free root) puts its first body: its geoms straddle the floor at small angles


def _one_hinge(B):
    B.body(-1, ["hinge"], pos=(0, 0, 0.5), limited=True)


def _one_slide(B):
    B.body(-1, ["slide"], ("sphere", "floor"), pos=(0, 0, 0.05), limited=True, axes=[(0.2, -0.1, 1.0)])


def _free_box(B):
    B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))


def _four_free(B):
    for k, g in enumerate(("sphere", "capsule", "capsule", "box")):
        B.body(-1, ["free"], (g, "all"), pos=(0.02 * k, 0, 0.3))


def _hinge_chain(n):
    def make(B):
        B.chain(-1, n, ("hinge",), first_pos=(0, 0, ROOT_Z))
        for i in range(max(1, n - 12), n):                         # geoms on the far bodies, which the joints before them lift and lower;
            B.bodies[i]["geom"] = B._geom(("capsule", "all") if i in (n - 6, n - 2) else ("sphere", "floor"))   # two meet each other
    return make


def _ball_chain(B):
    B.chain(-1, 10, ("ball",), geom_every=1, first_pos=(0, 0, ROOT_Z), step=(0.09, 0, 0))
    B.bodies[0]["geom"] = None


def _dofchain32(B):
    p = -1
    for k in range(8):                                             # (ball, hinge) x 8: one chain of 32 dofs, the last has 31 ancestors
        p = B.body(p, ["ball"], ("sphere", "floor") if k else None, pos=(0, 0, ROOT_Z) if k == 0 else (0.07, 0, 0))
        p = B.body(p, ["hinge"], ("capsule", "floor") if k % 2 else None)


def _bushy32(B):
    root = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))  # 6
    fan = [(0.08, 0, 0), (0, 0.08, 0), (-0.08, 0, 0), (0, -0.08, 0)]
    for c in range(4):                                             # 4 hinges, then 4 + 3 + 4 + 3 = 14 grandchildren, 4 of them balls: 6 + 4 + 10 + 12 = 32
        child = B.body(root, ["hinge"], ("capsule", "floor"), pos=fan[c])
        for g in range(4 if c % 2 == 0 else 3):
            step = np.array(fan[(c + g) % 4]) * 0.8 + np.array(fan[c]) * 0.5
            B.body(child, ["ball" if g == 0 else "hinge"], ("sphere", "floor"), pos=step)


def _nv33(B):
    root = B.body(-1, ["free"], ("sphere", "all"), pos=(0, 0, 0.3))
    for c, d in enumerate([(0.07, 0, 0), (-0.035, 0.06, 0), (-0.035, -0.06, 0)]):
        B.chain(root, 9, ("hinge",), geom_every=2, step=d)        # 6 + 27 = 33


def _nv38_other(B):
    root = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))
    for d in ((0, 0.07, 0), (0, -0.07, 0)):
        hip = B.body(root, ["ball"], ("sphere", "floor"), pos=d)
        B.chain(hip, 5, ("hinge",), geom_every=2, step=d)         # 2 x (3 + 5) = 16
    B.chain(root, 10, ("hinge",), geom_every=2)                    # + 10
    B.body(-1, ["free"], ("box", "all"), pos=(-0.05, 0, 0.3))     # + 6: 38; a second tree whose box meets the first's


def _nv40_full(B):
    r1 = B.body(-1, ["free"], ("capsule", "all"), pos=(0, 0, 0.3))
    for d in ((0.07, 0, 0), (-0.07, 0, 0)):
        B.chain(r1, 7, ("hinge",), geom_every=2, step=d)          # 6 + 14
    r2 = B.body(-1, ["free"], ("box", "all"), pos=(0, 0.3, 0.3))
    for d in ((0, 0.07, 0), (0, -0.07, 0)):
        hip = B.body(r2, ["ball"], ("sphere", "floor"), pos=d)
        B.chain(hip, 4, ("hinge",), geom_every=2, step=d)         # 6 + 2 x 7: 40 in all


def _bodies32(B):
    root = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))
    for d in ((0.06, 0, 0), (-0.03, 0.05, 0), (-0.03, -0.05, 0)):
        p = root
        for k in range(10):                                        # jointed and welded bodies in turn: 1 + 30 bodies, 6 + 15 dofs
            p = B.body(p, ["hinge"] if k % 2 == 0 else [], ("sphere", "floor") if k % 2 == 1 else None, pos=d)


def _nq48(B):
    root = B.body(-1, ["free"], ("sphere", "all"), pos=(0, 0, 0.3))           # 7
    tips = [B.chain(root, 3, ("ball",), geom_every=1, step=d) for d in ((0.08, 0, 0), (-0.04, 0.07, 0), (-0.04, -0.07, 0))]   # + 36
    B.chain(tips[0], 5, ("hinge",), geom_every=2)                              # + 5


def _multi_joint(B):
    a = B.body(-1, ["hinge", "hinge"], None, pos=(0, 0, ROOT_Z))
    b = B.body(a, ["slide", "hinge"], ("capsule", "floor"))
    c = B.body(b, ["hinge", "slide", "hinge"], ("sphere", "floor"))
    d = B.body(c, ["hinge", "hinge", "hinge"], ("box", "all"))
    B.body(d, ["hinge"], ("sphere", "floor"))
    B.body(a, ["slide", "slide", "hinge"], ("capsule", "all"), pos=(0, 0.07, 0))


def _pelvis_like(B):
    root = B.body(-1, ["slide", "slide", "slide", "ball"], ("box", "all"), pos=(0, 0, 0.3), limited=False,
                  axes=[(1, 0.1, 0), (0, 1, 0.1), (0.1, 0, 1), (0, 0, 1)])
    for d in ((0, 0.06, 0), (0, -0.06, 0)):
        B.chain(root, 3, ("hinge",), geom_every=1, step=d)


def _loops(B):
    r1 = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))
    tips = [B.chain(r1, 2, ("hinge",), geom_every=2, step=d) for d in ((0.07, 0, 0), (0, 0.07, 0), (-0.07, 0, 0), (0, -0.07, 0))]
    r2 = B.body(-1, ["free"], ("sphere", "all"), pos=(0, 0, 0.45))
    arms = [B.chain(r2, 2, ("hinge",), step=d) for d in ((0.07, 0, 0), (-0.07, 0, 0))]
    rnd = lambda: B.rng.uniform(-0.03, 0.03, 3)
    for k in range(4):                                             # loops inside the first tree: tip to the next branch's tip
        B.equalities.append((tips[k], tips[(k + 1) % 4], rnd()))
    B.equalities.append((tips[0] - 1, tips[2] - 1, rnd()))
    B.equalities.append((arms[0], arms[1], rnd()))                 # inside the second tree
    B.equalities.append((arms[0], tips[0], rnd()))                 # and between the trees
    B.equalities.append((r2, r1, rnd()))


def _actuated(B):
    root = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))
    k = 0
    for d in ((0.06, 0.05, 0), (0.06, -0.05, 0), (-0.06, 0.05, 0), (-0.06, -0.05, 0)):
        p = root
        for s in range(3):
            p = B.body(p, ["hinge"], ("sphere", "floor") if s != 1 else None, pos=d)
            B.motors.append((B.joint_name(p), (1.0, 25.0, 16.0, 50.0)[k % 4] * (1 + 0.1 * (k // 4)), float(B.rng.uniform(0.5, 4.0))))
            k += 1


def _sensed(B):
    root = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3), site=True)
    legs = [B.chain(root, 4, ("hinge",), geom_every=1, step=d, site_every=1) for d in ((0.07, 0, 0), (-0.07, 0, 0))]
    ball = B.body(root, ["ball"], ("sphere", "floor"), pos=(0, 0.07, 0), site=True)
    B.motors.append((B.joint_name(legs[0]), 25.0, 2.0))
    sites = ["s%d" % i for i, b in enumerate(B.bodies) if b["site"] is not None]     # 10 sites on 10 bodies
    assert len(sites) == 10 and ball == len(B.bodies) - 1
    # 1 + 2 * 1 + 4 * 4 + 4 * 3 + 2 * 3 + 3 = 40 = CM_MAXSENSORDATA
    B.sensors += ['<actuatorpos name="ap" actuator="m0"/>']
    B.sensors += ['<jointpos name="jp%d" joint="%s"/>' % (k, B.joint_name(b)) for k, b in enumerate((legs[1], legs[0] - 1))]
    B.sensors += ['<framequat name="fq%d" objtype="site" objname="%s"/>' % (k, sites[k]) for k in (0, 2, 5, 9)]
    B.sensors += ['<gyro name="gy%d" site="%s"/>' % (k, sites[k]) for k in (0, 3, 6, 9)]
    B.sensors += ['<accelerometer name="ac%d" site="%s"/>' % (k, sites[k]) for k in (0, 4)]
    B.sensors += ['<magnetometer name="mg" site="%s"/>' % sites[8]]


GENERIC32, GENERIC40 = 5, 6        # ck::StepFamily (csrc/step_plan.h)

# member -> (builder, what the loaded pod must show exactly: nv, nq, nbody (the world included), maxdepth, kin_simple; the rest of a
# member's facts -- the family and the padded size follow from nv -- are asserted from these)
MEMBERS = {
    "one_hinge":   (_one_hinge,       dict(nv=1, nq=1, nbody=2, maxdepth=1, kin_simple=1, ngeom=1)),
    "one_slide":   (_one_slide,       dict(nv=1, nq=1, nbody=2, maxdepth=1, kin_simple=1)),
    "free_box":    (_free_box,        dict(nv=6, nq=7, nbody=2, maxdepth=1, kin_simple=1, nroot=1)),
    "four_free":   (_four_free,       dict(nv=24, nq=28, nbody=5, maxdepth=1, kin_simple=1, nroot=4)),
    "chain27":     (_hinge_chain(27), dict(nv=27, nq=27, nbody=28, maxdepth=27, kin_simple=1)),
    "chain26":     (_hinge_chain(26), dict(nv=26, nq=26, nbody=27, maxdepth=26, kin_simple=1)),
    "chain9":      (_hinge_chain(9),  dict(nv=9, nq=9, nbody=10, maxdepth=9, kin_simple=1)),
    "ball_chain":  (_ball_chain,      dict(nv=30, nq=40, nbody=11, maxdepth=10, kin_simple=1)),
    "dofchain32":  (_dofchain32,      dict(nv=32, nq=40, nbody=17, maxdepth=16, kin_simple=1, dofdepth=31)),
    "bushy32":     (_bushy32,         dict(nv=32, nq=37, nbody=20, maxdepth=3, kin_simple=1, root_children=4)),
    "nv33":        (_nv33,            dict(nv=33, nq=34, nbody=29, maxdepth=10, kin_simple=1)),
    "nv38_other":  (_nv38_other,      dict(nv=38, nq=42, nbody=25, maxdepth=11, kin_simple=1, nroot=2)),
    "nv40_full":   (_nv40_full,       dict(nv=40, nq=44, nbody=27, maxdepth=8, kin_simple=1, nroot=2)),
    "bodies32":    (_bodies32,        dict(nv=21, nq=22, nbody=32, maxdepth=11, kin_simple=1)),
    "nq48":        (_nq48,            dict(nv=38, nq=48, nbody=16, maxdepth=9, kin_simple=1)),
    "multi_joint": (_multi_joint,     dict(nv=14, nq=14, nbody=7, maxdepth=5, kin_simple=0)),
    "pelvis_like": (_pelvis_like,     dict(nv=12, nq=13, nbody=8, maxdepth=4, kin_simple=1)),
    "loops":       (_loops,           dict(nv=24, nq=26, nbody=15, maxdepth=3, kin_simple=1, neq=8, nroot=2)),
    "actuated":    (_actuated,        dict(nv=18, nq=19, nbody=14, maxdepth=4, kin_simple=1, nu=12)),
    "sensed":      (_sensed,          dict(nv=17, nq=19, nbody=11, maxdepth=5, kin_simple=1, nsensor=14, nsensordata=40)),
}


def generate(member, directory, seed=0):
    """Writes the member's MJCF into `directory`; -> the file's path.  The text is a pure function of (member, seed)."""
    B = _Builder(member, seed)
    MEMBERS[member][0](B)
    path = os.path.join(str(directory), member + ".xml")
    with open(path, "w") as f:
        f.write(B.xml())
    return path


# ------------------------------------------------------------------------------------------------------------ the refusals
def _too_deep(B):
    B.chain(-1, 28, ("hinge",), first_pos=(0, 0, ROOT_Z))


def _dofchain33(B):
    B.chain(-1, 11, ("ball",), first_pos=(0, 0, ROOT_Z))


def _five_trees(B):
    for k in range(5):
        B.body(-1, ["free"], pos=(0.2 * k, 0, 0.3))


def _five_children(B):
    root = B.body(-1, ["free"], pos=(0, 0, 0.3))
    for k in range(5):
        B.body(root, ["hinge"], pos=(0.05 * k, 0.05, 0))


def _nv41(B):
    root = B.body(-1, ["free"], pos=(0, 0, 0.3))
    for d in ((0.07, 0, 0), (-0.07, 0, 0), (0, 0.07, 0)):
        B.chain(root, 9, ("hinge",), step=d)
    B.chain(root, 8, ("hinge",), step=(0, -0.07, 0))               # 6 + 27 + 8 = 41


def _nested_free(B):
    root = B.body(-1, ["free"], ("box", "all"), pos=(0, 0, 0.3))
    B.body(root, ["free"], ("sphere", "all"), pos=(0.1, 0, 0))


def _shared_free(B):
    B.body(-1, ["free", "hinge"], ("box", "all"), pos=(0, 0, 0.3))


# name -> (builder, a regular expression the loader's message must match)
REFUSALS = {
    "depth28":       (_too_deep,      r"kinematic tree deeper than 27 levels"),
    "dofchain33":    (_dofchain33,    r"dof chain deeper than 32"),
    "five_trees":    (_five_trees,    r"more than 4 kinematic trees"),
    "five_children": (_five_children, r"a body has more than 4 children"),
    "nv41":          (_nv41,          r"exceeds the compiled capacity limits"),
    "nested_free":   (_nested_free,   r"free joint j1_0 .*parent is not the world"),
    "shared_free":   (_shared_free,   r"free joint j0_0 .*shares its body"),
}


def generate_refusal(name, directory, seed=0):
    B = _Builder(name, seed)
    REFUSALS[name][0](B)
    path = os.path.join(str(directory), name + ".xml")
    with open(path, "w") as f:
        f.write(B.xml())
    return path


# ------------------------------------------------------------------------------------------------------------ the states
FREE, BALL, SLIDE, HINGE = range(4)


def _rand_quat(rng, n, near=None):
    q = rng.standard_normal((n, 4))
    if near is not None:
        q[near] = q[near] * 0.02 + [1, 0, 0, 0]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def sample_states(pod, n, seed=0):
    """-> (q [n][nq], v [n][nv], ctrl [n][nu]): hinges and slides across and 2 % past their ranges (+-0.7 about the reference where
    unlimited), ball and free orientations uniform on the sphere, free roots within 6 cm of their places (every fourth env: 48 cm), the lowest point of every tree that can be moved up and down (a free
    root, a root on slides) from free flight to 3 cm below the floor, every fourth env with small joint angles and upright roots so
    that everything lies near the floor, velocities up to +-5, ctrl up to 1.1 x the control range."""
    import family_ref
    rng = np.random.default_rng([int(seed), 77, pod.nv, pod.nq])
    q = np.tile(np.array(pod.qpos0[: pod.nq]), (n, 1))
    near = np.arange(n) % 4 == 3
    for j in range(pod.njnt):
        t, a = pod.jnt_type[j], pod.jnt_qposadr[j]
        if t in (HINGE, SLIDE):
            lo, hi = pod.jnt_range[j][0], pod.jnt_range[j][1]
            if pod.jnt_limited[j]:
                w = hi - lo
                q[:, a] = rng.uniform(lo - 0.02 * w, hi + 0.02 * w, n)
            else:
                q[:, a] = pod.qpos0[a] + rng.uniform(-0.7, 0.7, n) * (1.0 if t == HINGE else 0.3)
            small = pod.qpos0[a] + rng.standard_normal(n) * (0.03 if t == HINGE else 0.005)
            q[near, a] = small[near]
        elif t == BALL:
            q[:, a: a + 4] = _rand_quat(rng, n, near)
        else:
            q[:, a: a + 2] += rng.uniform(-0.06, 0.06, (n, 2)) * np.where(np.arange(n) % 4 == 1, 8.0, 1.0)[:, None]   # a quarter: trees apart
            q[:, a + 3: a + 7] = _rand_quat(rng, n, near)
    # heights: move every movable tree so that its lowest point sits where the draw says
    want = np.where(rng.random(n) < 0.5, rng.uniform(-0.03, 0.0, n), np.where(rng.random(n) < 0.5, rng.uniform(0.0, 0.04, n), rng.uniform(0.04, 0.5, n)))
    want[near] = rng.uniform(-0.012, -0.004, int(near.sum()))
    for e in range(n):
        kin = family_ref.kinematics(pod, q[e], dtype=np.float64)
        low = family_ref.lowest_points(pod, kin)
        for r in range(pod.nroot):
            root = pod.root_body[r]
            if not np.isfinite(low[root]):
                continue
            dz = want[e] - low[root]
            j0, jn = pod.body_jntadr[root], pod.body_jntnum[root]
            if jn == 1 and pod.jnt_type[j0] == FREE:
                q[e, pod.jnt_qposadr[j0] + 2] += dz
            else:
                slides = [j for j in range(j0, j0 + jn) if pod.jnt_type[j] == SLIDE and not pod.jnt_limited[j]]
                if len(slides) == 3:                               # three slides ahead of the rotation: the least-norm shift that lifts by dz
                    az = np.array([kin["jnt_axis"][j][2] for j in slides])
                    for j, d in zip(slides, dz * az / (az @ az)):
                        q[e, pod.jnt_qposadr[j]] += d
                    kin2 = family_ref.kinematics(pod, q[e], dtype=np.float64)
                    assert abs(family_ref.lowest_points(pod, kin2)[root] - want[e]) < 1e-9
    v = rng.uniform(-5.0, 5.0, (n, pod.nv))
    hi = np.array([pod.act_ctrlrange[u][1] for u in range(pod.nu)])
    ctrl = rng.uniform(-1.1, 1.1, (n, pod.nu)) * hi
    return q, v, ctrl
