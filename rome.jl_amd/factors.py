"""Host-side mirror of the RoME.jl factor / variable plugin surface for the hot path.

Same names and argument meaning as the reference (paths relative to the RoME.jl checkout):
  variable types  Pose2, Point2, Pose3                       src/variables/VariableTypes.jl:13,35,47
  Pose2Pose2(Z)                                              src/factors/Pose2D.jl:30-32
  PriorPose2(Z)                                              src/factors/PriorPose2.jl:13-15
  Pose2Point2BearingRange(bearing, range)                    src/factors/BearingRange2D.jl:10-13
  Pose3Pose3(Z), PriorPose3(Z)                               src/factors/Pose3Pose3.jl:9-11, Pose3D.jl:8-10
  Point2Point2Range(Z), Pose2Point2Range(Z)                 src/factors/Range2D.jl:8-17, 40-54
  Pose2Point2Bearing(Z)                                      src/factors/Bearing2D.jl:10-32
  Pose3Pose3XYYaw(Z), PriorPose3ZRP(z, rp)                   src/factors/PartialPose3.jl:101-136, 12-46
  Pose3Pose3Rotation(Z)                                      src/factors/PartialPose3.jl:204-227
  getMeasurementParametric(::Pose2Point2BearingRange)        src/factors/BearingRange2D.jl:30-37
  Packed* <-> factor converters                              src/factors/Pose2D.jl:76-84 etc.
These objects only hold the measurement model; all arithmetic is done by the HIP library.
"""
import numpy as np


# ---- minimal stand-ins for Distributions.jl beliefs the hot-path factors are built from ----
class MvNormal:
    """MvNormal(μ, Σ) -- Σ may be a full matrix or a vector of the diagonal (like Diagonal(...))."""

    def __init__(self, mu, cov=None):
        mu = np.asarray(mu, dtype=np.float64)
        if cov is None:  # MvNormal(Σ) zero-mean form (Pose2D.jl:31 default)
            cov = mu
            cov = np.asarray(cov, dtype=np.float64)
            mu = np.zeros(cov.shape[0])
        cov = np.asarray(cov, dtype=np.float64)
        if cov.ndim == 1:
            cov = np.diag(cov)
        if cov.shape != (mu.size, mu.size):
            raise ValueError("MvNormal: covariance shape %s does not match mean of length %d" % (cov.shape, mu.size))
        self.mu = mu
        self.cov = cov

    def __repr__(self):
        return "FullNormal(dim: %d μ: %s Σ: %s)" % (self.mu.size, self.mu.tolist(), self.cov.tolist())


class Normal:
    def __init__(self, mu=0.0, sigma=1.0):
        if not sigma >= 0:
            raise ValueError("Normal: sigma must be non-negative")
        self.mu = float(mu)
        self.sigma = float(sigma)

    def __repr__(self):
        return "Normal(μ=%r, σ=%r)" % (self.mu, self.sigma)


class Uniform:
    """Uniform(a, b) (Distributions.jl); accepted for the bearing / range beliefs of Pose2Point2BearingRange."""

    def __init__(self, a, b):
        if not b > a:
            raise ValueError("Uniform: need a < b")
        self.a, self.b = float(a), float(b)
        self.mu = 0.5 * (self.a + self.b)
        self.sigma = -0.5 * (self.b - self.a)   # library encoding: negative "sigma" = half-width of a uniform

    def __repr__(self):
        return "Uniform(a=%r, b=%r)" % (self.a, self.b)


# ---- variable types ----
class _VarType:
    dim = 0        # manifold dimension (tangent coordinates)
    point_len = 0  # doubles in the reference's native point representation
    name = ""

    def __repr__(self):
        return self.name


class _Pose2(_VarType):
    dim, point_len, name = 3, 6, "Pose2"


class _Point2(_VarType):
    dim, point_len, name = 2, 2, "Point2"


class _Pose3(_VarType):
    dim, point_len, name = 6, 12, "Pose3"


Pose2, Point2, Pose3 = _Pose2(), _Point2(), _Pose3()


# ---- factors ----
class _RelativeFactor:
    """<: IIF.AbstractManifoldMinimize"""
    is_prior = False


class _PriorFactor:
    """<: IIF.AbstractPrior"""
    is_prior = True


class Pose2Pose2(_RelativeFactor):
    variable_types = (Pose2, Pose2)

    def __init__(self, Z=None):
        self.Z = Z if Z is not None else MvNormal(np.zeros(3), np.eye(3))  # Pose2D.jl:31
        if self.Z.mu.size != 3:
            raise ValueError("Pose2Pose2 needs a 3-dimensional belief")


class PriorPose2(_PriorFactor):
    variable_types = (Pose2,)

    def __init__(self, Z=None):
        self.Z = Z if Z is not None else MvNormal(np.zeros(3), np.diag([1, 1, 0.1]))  # PriorPose2.jl:14
        if self.Z.mu.size != 3:
            raise ValueError("PriorPose2 needs a 3-dimensional belief")


class Pose2Point2BearingRange(_RelativeFactor):
    variable_types = (Pose2, Point2)

    def __init__(self, bearing, range):  # noqa: A002  (mirrors the reference field name)
        if not isinstance(bearing, (Normal, Uniform)) or not isinstance(range, (Normal, Uniform)):
            raise TypeError("Pose2Point2BearingRange: this build supports Normal / Uniform bearing and range beliefs")
        self.bearing = bearing
        self.range = range


class Pose3Pose3(_RelativeFactor):
    variable_types = (Pose3, Pose3)

    def __init__(self, Z=None):
        self.Z = Z if Z is not None else MvNormal(np.zeros(6), np.diag([0.01] * 3 + [0.0001] * 3))  # Pose3Pose3.jl:10
        if self.Z.mu.size != 6:
            raise ValueError("Pose3Pose3 needs a 6-dimensional belief")


class PriorPose3(_PriorFactor):
    variable_types = (Pose3,)

    def __init__(self, Z=None):
        self.Z = Z if Z is not None else MvNormal(np.zeros(6), np.diag([0.01] * 3 + [0.0001] * 3))  # Pose3D.jl:9
        if self.Z.mu.size != 6:
            raise ValueError("PriorPose3 needs a 6-dimensional belief")


class PriorPoint2(_PriorFactor):
    """Direction observation information of a `Point2` variable (src/factors/Point2D.jl:9-18).  Only the
    parametric path uses it here (it anchors landmarks in the reference's parametric tests)."""
    variable_types = (Point2,)

    def __init__(self, Z=None):
        self.Z = Z if Z is not None else MvNormal(np.zeros(2), np.diag([0.01, 0.01]))  # Point2D.jl:10
        if self.Z.mu.size != 2:
            raise ValueError("PriorPoint2 needs a 2-dimensional belief")


class Point2Point2(_RelativeFactor):
    """Translation between two `Point2` variables (src/factors/Point2D.jl:23-43).  Host-side type only: the box
    generator builds graphs with it; it is not one of the hot-path factor kinds, so packing a graph that holds one for
    the device raises."""
    variable_types = (Point2, Point2)

    def __init__(self, Z=None):
        self.Z = Z if Z is not None else MvNormal(np.zeros(2), np.eye(2))
        if self.Z.mu.size != 2:
            raise ValueError("Point2Point2 needs a 2-dimensional belief")


class Point2Point2Range(_RelativeFactor):
    """Range between two `Point2` variables (src/factors/Range2D.jl:8-17): r = ρ − ‖lm − xi‖ over [xi, lm].  Z is a `Normal` or a
    `Uniform` belief of the range.  One range constrains the other point to a ring: the convolution keeps the start point's member of
    it (every solver runs the inflation cycles)."""
    variable_types = (Point2, Point2)

    def __init__(self, Z):
        if not isinstance(Z, (Normal, Uniform)):
            raise TypeError("Point2Point2Range: this build supports a Normal / Uniform range belief, got %s" % type(Z).__name__)
        self.Z = Z


class Pose2Point2Range(_RelativeFactor):
    """Range from a `Pose2` to a `Point2` (src/factors/Range2D.jl:40-54): r = ρ − ‖lm − x.t‖ over [x, lm], partial = (1, 2) on the
    pose (:44).  Solving the pose moves its (x, y) only; every particle's heading passes through unchanged."""
    variable_types = (Pose2, Point2)
    partial = (1, 2)

    def __init__(self, Z):
        if not isinstance(Z, (Normal, Uniform)):
            raise TypeError("Pose2Point2Range: this build supports a Normal / Uniform range belief, got %s" % type(Z).__name__)
        self.Z = Z


class Pose2Point2Bearing(_RelativeFactor):
    """Bearing from a `Pose2` to a `Point2` and no distance (src/factors/Bearing2D.jl:10-32): r = sym_rem(b − atan2(pl)),
    pl = R(θp)ᵀ (l − p.t) over [p, l].  Z is a `Normal` or a `Uniform` belief of the bearing (default Normal(), :15).  One bearing
    leaves the landmark on a ray from the pose and the pose on a two-parameter family: the convolution keeps the start point's
    distance (landmark) or translation (pose) and every solver runs the inflation cycles."""
    variable_types = (Pose2, Point2)

    def __init__(self, Z=None):
        Z = Normal() if Z is None else Z
        if not isinstance(Z, (Normal, Uniform)):
            raise TypeError("Pose2Point2Bearing: this build supports a Normal / Uniform bearing belief, got %s" % type(Z).__name__)
        self.Z = Z


class Pose3Pose3XYYaw(_RelativeFactor):
    """Planar odometry with heading between two `Pose3` variables (src/factors/PartialPose3.jl:101-136), partial = (1, 2, 6): the
    Pose2Pose2 residual of the two poses' SE(2) projections (t_xy, yaw).  Solving a pose moves its (x, y, ω_z) only; every particle's
    z, ω_x, ω_y pass through unchanged."""
    variable_types = (Pose3, Pose3)
    partial = (1, 2, 6)

    def __init__(self, Z):
        if not isinstance(Z, MvNormal):
            raise TypeError("Pose3Pose3XYYaw: this build supports an MvNormal belief, got %s" % type(Z).__name__)
        if Z.mu.size != 3:
            raise ValueError("Pose3Pose3XYYaw needs a 3-dimensional belief (x, y, yaw)")
        self.Z = Z


class PriorPose3ZRP(_PriorFactor):
    """Partial prior on z, roll and pitch of a `Pose3` (src/factors/PartialPose3.jl:12-46), partial = (3, 4, 5): z a `Normal`, rp a
    2-dimensional `MvNormal` of (roll, pitch).  The proposal is the variable's own belief with coordinates 3, 4, 5 replaced by the
    samples (z, and ω_x, ω_y of Log(R_y(pitch) R_x(roll))); x, y, ω_z pass through unchanged."""
    variable_types = (Pose3,)
    partial = (3, 4, 5)

    def __init__(self, z, rp):
        if not isinstance(z, Normal):
            raise TypeError("PriorPose3ZRP: this build supports a Normal z belief, got %s" % type(z).__name__)
        if not isinstance(rp, MvNormal):
            raise TypeError("PriorPose3ZRP: this build supports an MvNormal roll / pitch belief, got %s" % type(rp).__name__)
        if rp.mu.size != 2:
            raise ValueError("PriorPose3ZRP needs a 2-dimensional roll / pitch belief")
        self.z = z
        self.rp = rp


class Pose3Pose3Rotation(_RelativeFactor):
    """Relative attitude between two `Pose3` variables (src/factors/PartialPose3.jl:204-227), partial = (4, 5, 6): r = Z − Log(R_pᵀ R_q),
    Z a 3-dimensional `MvNormal` of the rotation vector.  Solving a pose moves its (ω_x, ω_y, ω_z) only; every particle's translation
    passes through unchanged."""
    variable_types = (Pose3, Pose3)
    partial = (4, 5, 6)

    def __init__(self, Z):
        if not isinstance(Z, MvNormal):
            raise TypeError("Pose3Pose3Rotation: this build supports an MvNormal belief, got %s" % type(Z).__name__)
        if Z.mu.size != 3:
            raise ValueError("Pose3Pose3Rotation needs a 3-dimensional belief (the rotation vector)")
        self.Z = Z


RANGE_FACTORS = (Point2Point2Range, Pose2Point2Range)
PARTIAL3_FACTORS = (Pose3Pose3XYYaw, PriorPose3ZRP, Pose3Pose3Rotation)


def partial_coverage(factor, position):
    """0-based coordinates of the variable at `position` of `factor` (a factor or a factor class) that its proposal towards that
    variable solves, or None when it solves all of them.  From the `partial` class attributes (1-based, as in the reference); the
    `partial` of Pose2Point2Range is on the pose alone (Range2D.jl:44): its proposal towards the landmark is full."""
    cls = factor if isinstance(factor, type) else type(factor)
    p = getattr(cls, "partial", None)
    if p is None or (cls is Pose2Point2Range and position != 0):
        return None
    cover = tuple(int(k) - 1 for k in p)
    return None if len(cover) == cls.variable_types[position].dim else cover


def refuse_range(factors, where):
    """TypeError naming the first range-only factor in `factors` (paths that do not serve them yet)."""
    for f in factors:
        if isinstance(f, RANGE_FACTORS):
            raise TypeError("%s: %s factors are not supported here (solveGraph / approxConv serve range factors)"
                            % (where, type(f).__name__))


def refuse_bearing(factors, where):
    """TypeError naming the first bearing-only factor in `factors` (the paths that refuse range factors refuse these too)."""
    for f in factors:
        if isinstance(f, Pose2Point2Bearing):
            raise TypeError("%s: Pose2Point2Bearing factors are not supported here (solveGraph / approxConv / solveGraphParametric "
                            "serve bearing-only factors)" % where)


def refuse_partial3(factors, where):
    """TypeError naming the first partial Pose3 factor in `factors` (the paths that refuse range factors refuse these too)."""
    for f in factors:
        if isinstance(f, PARTIAL3_FACTORS):
            raise TypeError("%s: %s factors are not supported here (solveGraph / approxConv serve the partial Pose3 factors)"
                            % (where, type(f).__name__))


def refuse_unserved(factors, where):
    """the three refusals of the paths that serve none of these families: range, bearing-only, partial Pose3, in that order"""
    refuse_range(factors, where)
    refuse_bearing(factors, where)
    refuse_partial3(factors, where)


def getMeasurementParametric(f):
    """(μ, iΣ) as IIF.getMeasurementParametric; BearingRange override at BearingRange2D.jl:30-37."""
    if isinstance(f, Pose2Point2Bearing):
        if not isinstance(f.Z, Normal):
            raise TypeError("getMeasurementParametric(::Pose2Point2Bearing{<:Normal}) only")
        return np.array([f.Z.mu]), np.array([[1.0 / f.Z.sigma ** 2]])
    if isinstance(f, Pose2Point2BearingRange):
        if not isinstance(f.bearing, Normal) or not isinstance(f.range, Normal):
            raise TypeError("getMeasurementParametric(::Pose2Point2BearingRange{<:Normal,<:Normal}) only (BearingRange2D.jl:30)")
        return (np.array([f.bearing.mu, f.range.mu]),
                np.diag([1.0 / f.bearing.sigma ** 2, 1.0 / f.range.sigma ** 2]))
    return f.Z.mu.copy(), np.linalg.inv(f.Z.cov)


# ---- Packed* serialisation (dict form of the reference's Packed structs) ----
def _pack_belief(b):
    if isinstance(b, Normal):
        return {"_type": "Normal", "mu": b.mu, "sigma": b.sigma}
    if isinstance(b, Uniform):
        return {"_type": "Uniform", "a": b.a, "b": b.b}
    return {"_type": "FullNormal", "mu": b.mu.tolist(), "cov": b.cov.tolist()}


def _unpack_belief(d):
    if d["_type"] == "Normal":
        return Normal(d["mu"], d["sigma"])
    if d["_type"] == "Uniform":
        return Uniform(d["a"], d["b"])
    return MvNormal(d["mu"], np.asarray(d["cov"]))


def pack_factor(f):
    name = type(f).__name__
    if isinstance(f, Pose2Point2BearingRange):  # PackedPose2Point2BearingRange: bearstr, rangstr (BearingRange2D.jl:76-79)
        return {"fnctype": name, "bearstr": _pack_belief(f.bearing), "rangstr": _pack_belief(f.range)}
    if isinstance(f, PriorPose3ZRP):  # PackedPriorPose3ZRP: zdata, rpdata (PartialPose3.jl:54-57)
        return {"fnctype": name, "zdata": _pack_belief(f.z), "rpdata": _pack_belief(f.rp)}
    return {"fnctype": name, "Z": _pack_belief(f.Z)}


def unpack_factor(d):
    t = d["fnctype"]
    if t == "Pose2Point2BearingRange":
        return Pose2Point2BearingRange(_unpack_belief(d["bearstr"]), _unpack_belief(d["rangstr"]))
    if t == "PriorPose3ZRP":
        return PriorPose3ZRP(_unpack_belief(d["zdata"]), _unpack_belief(d["rpdata"]))
    cls = {"Pose2Pose2": Pose2Pose2, "PriorPose2": PriorPose2, "Pose3Pose3": Pose3Pose3, "PriorPose3": PriorPose3,
           "PriorPoint2": PriorPoint2, "Point2Point2Range": Point2Point2Range, "Pose2Point2Range": Pose2Point2Range,
           "Pose2Point2Bearing": Pose2Point2Bearing,    # PackedPose2Point2Bearing: Z (Bearing2D.jl:36-45)
           "Pose3Pose3XYYaw": Pose3Pose3XYYaw,          # PackedPose3Pose3XYYaw: Z (PartialPose3.jl:172-174)
           "Pose3Pose3Rotation": Pose3Pose3Rotation}[t]  # PackedPose3Pose3Rotation: Z (PartialPose3.jl:234-236)
    return cls(_unpack_belief(d["Z"]))


# ---- point <-> coordinate layout helpers (host-side format conversion only) ----
def getPoint(vartype, coords):
    """exp_ϵ(hat(c)) in the reference's native point layout (column-major R)."""
    c = np.asarray(coords, dtype=np.float64)
    if vartype is Pose2:
        s, co = np.sin(c[..., 2]), np.cos(c[..., 2])
        return np.stack([c[..., 0], c[..., 1], co, s, -s, co], axis=-1)
    if vartype is Point2:
        return c.copy()
    if vartype is Pose3:
        from scipy.spatial.transform import Rotation as Rot
        R = Rot.from_rotvec(c[..., 3:].reshape(-1, 3)).as_matrix()  # (n,3,3)
        Rcm = np.transpose(R, (0, 2, 1)).reshape(c.shape[:-1] + (9,))
        return np.concatenate([c[..., :3], Rcm], axis=-1)
    raise TypeError(vartype)


def getCoordinates(vartype, pt):
    """vee(log(ϵ, p))"""
    p = np.asarray(pt, dtype=np.float64)
    if vartype is Pose2:
        return np.stack([p[..., 0], p[..., 1], np.arctan2(p[..., 3], p[..., 2])], axis=-1)
    if vartype is Point2:
        return p.copy()
    if vartype is Pose3:
        from scipy.spatial.transform import Rotation as Rot
        R = np.transpose(p[..., 3:].reshape(-1, 3, 3), (0, 2, 1))
        w = Rot.from_matrix(R).as_rotvec().reshape(p.shape[:-1] + (3,))
        return np.concatenate([p[..., :3], w], axis=-1)
    raise TypeError(vartype)
