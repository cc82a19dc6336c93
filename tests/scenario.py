"""A synthetic closed-loop scenario for prediction.FaceTracker whose truth exists outside the package's own statement of
itself: an analytic texture, faces posed by known similarities (or a known 3-D rotation), frames rendered from them in
float64, and a stand-in for the landmark model that returns the truth landmarks through the tracker's CURRENT crop
matrices.  numpy float64 throughout; only `TruthSource` touches torch.

Coordinates.  FACE coordinates (u, v) are the pixels of the aligned face (OUT x OUT), so the aligned template is
`alignment.canonical_template(68, OUT, OUT)` and a face seen through the inverse of its own pose is tex(u, v) itself.  FRAME
coordinates (x, y) put pixel (row i, column j) at (x, y) = (j, i), as every warp of the package does.

Texture.  tex(u, v)[c] = 128 + sum_k A_k G_kc sin(wx_k u + wy_k v + p_k): it can be evaluated anywhere, a Gaussian blur of
sigma s (in face px) scales term k by exp(-s^2 |w_k|^2 / 2) exactly, and the per-channel gains G_kc differ, so B and R are
not interchangeable.  Every expectation is a closed form: no interpolation, no resampling of a stored image.

Cast (2 streams x 4 slots, frames of 270 x 480, TICKS ticks, a detector every KEY-th tick):
  stream 0: P0 (slot 0) moves right, P1 (slot 1) moves left; they pass each other at half time, one above the other, and
            the detector lists its boxes by ascending x, so the order of the detections swaps there;
  stream 1: H (slot 4), the head: the six landmarks of the package's HeadModel are the weak-perspective projection of its
            3-D points under the scripted yaw, pitch, roll, scale and shift (the other 62 landmarks are the template lifted
            onto a bowl and projected the same way); yaw sweeps through both edges of PoseViews(); its pixels are the
            planar texture at the float64 Umeyama fit of its 68 landmarks;
            P2 (slot 5) drifts, then leaves through the right edge: at tick P2_EXIT its crop centre is past the last
            column and the step reports TRACK_OUTSIDE; P3 is born in the same slot at tick P3_BIRTH.
Slots 2, 3, 6 and 7 never hold a face.

What is left out: `step_active` and `step_live` hand the model ROWS gathered from the slots, and which slot a row serves
is known only to the private snapshot of those calls; `TruthSource` reads the public `m_crop` of all slots, so it serves
`step` alone (and `step_flow`, which does not call the model).  The row forms are not part of this scenario."""
import math

import numpy as np

import flm_amd  # noqa: F401
from flm_amd import alignment

f64 = np.float64
FH, FW, TICKS, KEY = 270, 480, 32, 4
STREAMS, SLOTS, CAP = 2, 4, 8
IN, GRID, C, OUT = 64, 72, 68, 24
TEMPLATE = alignment.canonical_template(C, OUT, OUT)
CROP_TEMPLATE = alignment.canonical_template(C, IN, IN)
CENTRE = np.array([(OUT - 1) / 2.0, (OUT - 1) / 2.0])
PATCH = (-2.5, OUT - 1 + 2.5)          # the face coordinates a face paints: the aligned square with room for a tick's motion
BACKGROUND = np.array([96.0, 104.0, 112.0])
SHARP_REF = 16000.0                    # above the sharpness of every aligned face: the quality never saturates
SCORE_RECORD = (1.0, 0.25, 0.5, 0.125)  # score, var_x, var_y, cov_xy of every landmark record the source returns
P2_EXIT, P3_BIRTH = 12, 16
FLOW_RADIUS = 7                        # the window radius of alignment.LandmarkFlow()
E_REF = 0.36                           # crop px: the bar tests/test_scenario_host.py holds the measured e_ref under

# amplitude, (wx, wy) in rad per face px, phase, gains (B, G, R)
TERMS = ((40.0, (1.20, 1.10), 0.3, (0.75, 1.00, 0.55)),
         (30.0, (-0.50, 0.42), 1.1, (1.00, 0.70, 0.50)),
         (24.0, (0.30, 0.34), 2.0, (0.50, 0.80, 1.00)))


def tex(u, v, s=0.0):
    """The texture blurred by a Gaussian of sigma s face px, at any real (u, v): float64 [..., 3] (B, G, R)."""
    u, v = np.asarray(u, f64), np.asarray(v, f64)
    out = np.full(u.shape + (3,), 128.0)
    for a, (wx, wy), p, g in TERMS:
        k = a * math.exp(-0.5 * s * s * (wx * wx + wy * wy))
        out += (k * np.sin(wx * u + wy * v + p))[..., None] * np.asarray(g)
    return out


def curvature(s):
    """A bound of |f_dd| + |f_ee| over any two orthogonal unit directions d, e of face space, for the worst channel:
    sum_k A_k G_kc |w_k|^2 exp(-s^2 |w_k|^2 / 2), since |d^2/dd^2 sin(w.p)| <= (w.d)^2 and (w.d)^2 + (w.e)^2 = |w|^2."""
    tot = np.zeros(3)
    for a, (wx, wy), _, g in TERMS:
        w2 = wx * wx + wy * wy
        tot += a * math.exp(-0.5 * s * s * w2) * w2 * np.asarray(g)
    return float(tot.max())


def b_align(s, scale):
    """The bound of an aligned pixel against the float64 rendering: 0.5 for the uint8 rounding of the frame (a bilinear
    blend of four values that are each off by at most 0.5), plus the bilinear interpolation error of a C^2 function on
    a unit cell, (|f_xx| + |f_yy|) / 8 in frame px -- the face-space curvature over scale^2, scale being frame px per
    face px --, plus half a float32 ulp of a value below 256 for the output type."""
    return 0.5 + curvature(s) / (8.0 * scale * scale) + 2.0 ** -17


def umeyama(p, q):
    """The least-squares similarity p -> q of two [N,2] point sets in float64: (a, b, tx, ty) of [[a,-b,tx],[b,a,ty]],
    the closed form tests/stats_ref.py restates term by term."""
    p, q = np.asarray(p, f64), np.asarray(q, f64)
    mp, mq = p.mean(0), q.mean(0)
    pc, qc = p - mp, q - mq
    var = (pc * pc).sum()
    a = (pc * qc).sum() / var
    b = (pc[:, 0] * qc[:, 1] - pc[:, 1] * qc[:, 0]).sum() / var
    return np.array([a, b, mq[0] - (a * mp[0] - b * mp[1]), mq[1] - (b * mp[0] + a * mp[1])])


def matrix(sim):
    a, b, tx, ty = sim
    return np.array([[a, -b, tx], [b, a, ty]], f64)


def inverse(m):
    """The inverse of a [2,3] affine, float64."""
    m = np.asarray(m, f64)
    lin = np.linalg.inv(m[:, :2])
    return np.concatenate([lin, -(lin @ m[:, 2])[:, None]], 1)


def apply(m, pts):
    m = np.asarray(m, f64)
    return np.asarray(pts, f64) @ m[:, :2].T + m[:, 2]


def rotation(yaw, pitch, roll):
    """Rz(roll) Rx(pitch) Ry(yaw) in the model frame of include/flm.h (X right, Y down, Z away): the third row is
    (-cos(pitch) sin(yaw), sin(pitch), cos(pitch) cos(yaw)), which is what the head-pose record's angles are read from."""
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    rz = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]])
    return rz @ rx @ ry


def _hinge(t):
    return 0.5 * ((t - 2.0) + math.sqrt((t - 2.0) ** 2 + 4.0))


def _blur_c(i, t):
    """The blur of an ordinary tick: between 1.6 and 1.7 face px, different at every tick of a face."""
    return 1.6 + 0.1 * ((0.6180339887 * (7 * i + 13 * t + 1)) % 1.0)


class Face:
    """One face of the cast.  pose(t) -> S_t, the float64 [2,3] affine face px -> frame px; landmarks(t) -> [68,2]."""

    def __init__(self, name, index, stream, slot, first, last, sharp):
        self.name, self.index, self.stream, self.slot = name, index, stream, slot
        self.first, self.last = first, last          # the ticks the tracker holds it: `last` still returns a face
        self.sharp = dict(sharp)                      # tick -> blur, the ticks that are not ordinary: each starts at a `step`
        self._pose = {}

    @property
    def global_slot(self):
        return self.stream * SLOTS + self.slot

    def live(self, t):
        return self.first <= t <= self.last

    def rendered(self, t):
        return t >= self.first

    def blur(self, t):
        return self.sharp.get(t, _blur_c(self.index, t))

    def pose(self, t):
        if t not in self._pose:
            self._pose[t] = self._make(t)
        return self._pose[t][0]

    def landmarks(self, t):
        self.pose(t)
        return self._pose[t][1]

    def scale(self, t):
        m = self.pose(t)
        return math.hypot(m[0, 0], m[1, 0])


class Planar(Face):
    def __init__(self, *a, centre, angle, size):
        super().__init__(*a)
        self._centre, self._angle, self._size = centre, angle, size

    def _make(self, t):
        th, sc = self._angle(t), self._size(t)
        lin = sc * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        m = np.concatenate([lin, (np.asarray(self._centre(t), f64) - lin @ CENTRE)[:, None]], 1)
        return m, apply(m, TEMPLATE)


HEAD_INDICES = [int(i) for i in alignment.HeadModel.default(C).indices]
HEAD_POINTS = np.array(alignment.HeadModel.default(C).points, f64)


def head_shape():
    """A 3-D position for each of the 68 landmarks, in the units of the package's HeadModel: the model's own six points
    where it has one; elsewhere the template, scaled about the nose tip so that the outer eye corners and the chin keep
    the model's distances, lifted onto a bowl."""
    nose = TEMPLATE[30]
    sx = (TEMPLATE[45, 0] - TEMPLATE[36, 0]) / 450.0
    sy = (TEMPLATE[8, 1] - nose[1]) / 330.0
    xy = (TEMPLATE - nose) / np.array([sx, sy])
    z = np.minimum(0.0012 * (xy ** 2).sum(1), 200.0)
    pts = np.concatenate([xy, z[:, None]], 1)
    pts[HEAD_INDICES] = HEAD_POINTS
    return pts


class Head(Face):
    def __init__(self, *a, angles, size, shift):
        super().__init__(*a)
        self.angles, self._size, self._shift = angles, size, shift
        self._shape = head_shape()

    def _make(self, t):
        r = rotation(*self.angles(t))
        q = self._shape @ r.T
        lm = self._size(t) * q[:, :2] + np.asarray(self._shift(t), f64)
        return inverse(matrix(umeyama(lm, TEMPLATE))), lm


def _deg(x):
    return x * math.pi / 180.0


def head_angles(t):
    return (_deg(38.0) * math.sin(math.pi * (t - 15.97) / 31.0), _deg(8.0) * math.sin(0.3 * t), _deg(5.0) + _deg(2.0) * math.cos(0.25 * t))


def cast():
    return [
        Planar("P0", 0, 0, 0, 0, TICKS - 1, {8: 0.0, 9: 0.72},
               centre=lambda t: (170.0 + 4.0 * t, 66.0 + 3.0 * math.sin(0.4 * t)),
               angle=lambda t: _deg(6.0) + _deg(3.0) * math.sin(0.2 * t), size=lambda t: 85.0 / (OUT - 1) * (1 + 0.04 * math.sin(0.15 * t))),
        Planar("P1", 1, 0, 1, 0, TICKS - 1, {20: 0.0, 21: 0.72},
               centre=lambda t: (310.0 - 4.0 * t, 204.0 + 3.0 * math.sin(0.4 * t + 1.0)),
               angle=lambda t: -_deg(5.0) - _deg(3.0) * math.cos(0.23 * t), size=lambda t: 87.0 / (OUT - 1) * (1 + 0.04 * math.cos(0.17 * t))),
        Head("H", 2, 1, 0, 0, TICKS - 1, {4: 0.8, 16: 0.0, 17: 0.72, 28: 0.8}, angles=head_angles,
             size=lambda t: 0.1003 * (1 + 0.03 * math.sin(0.2 * t)),
             shift=lambda t: (115.0 + 12.0 * math.cos(0.25 * t), 150.0 + 12.0 * math.sin(0.25 * t))),
        Planar("P2", 3, 1, 1, 0, P2_EXIT, {0: 0.0, 1: 0.72},
               centre=lambda t: (424.0 + 5.6 * _hinge(t), 120.0 + 2.2 * t),
               angle=lambda t: _deg(5.0) + _deg(2.0) * math.sin(0.3 * t), size=lambda t: 84.0 / (OUT - 1)),
        Planar("P3", 4, 1, 1, P3_BIRTH, TICKS - 1, {24: 0.0, 25: 0.72},
               centre=lambda t: (300.0 - 2.5 * (t - P3_BIRTH), 90.0 + 2.8 * (t - P3_BIRTH)),
               angle=lambda t: -_deg(4.0) - _deg(2.0) * math.sin(0.3 * t), size=lambda t: 84.0 / (OUT - 1) * (1 + 0.03 * math.sin(0.2 * t))),
    ]


class Script:
    """The scenario: the cast, the frames, the detections and what the tracker must end up holding."""

    def __init__(self):
        self.faces = cast()
        self._frames = None

    def face_in(self, slot, t):
        """The face the global slot holds through tick t, or None."""
        for f in self.faces:
            if f.global_slot == slot and f.live(t):
                return f
        return None

    def is_key(self, t):
        return t % KEY == 0

    # ---- pixels ---------------------------------------------------------------------------------------------------------
    def scene(self, stream, t, x, y):
        """The continuous picture of a stream at tick t at any real frame points: float64 [..., 3].  A point outside the
        frame shows what the frame's edge shows (the warps clamp their taps)."""
        x = np.clip(np.asarray(x, f64), 0.0, FW - 1.0)
        y = np.clip(np.asarray(y, f64), 0.0, FH - 1.0)
        out = np.broadcast_to(BACKGROUND, x.shape + (3,)).copy()
        for f in self.faces:
            if f.stream != stream or not f.rendered(t):
                continue
            inv = inverse(f.pose(t))
            u = inv[0, 0] * x + inv[0, 1] * y + inv[0, 2]
            v = inv[1, 0] * x + inv[1, 1] * y + inv[1, 2]
            inside = (u >= PATCH[0]) & (u <= PATCH[1]) & (v >= PATCH[0]) & (v <= PATCH[1])
            if inside.any():
                out[inside] = tex(u[inside], v[inside], f.blur(t))
        return out

    def frame(self, stream, t):
        yy, xx = np.mgrid[0:FH, 0:FW].astype(f64)
        return np.clip(np.rint(self.scene(stream, t, xx, yy)), 0, 255).astype(np.uint8)

    def frames(self):
        """uint8 [STREAMS*TICKS, FH, FW, 3]: the ring; the frame of stream s at tick t lies in slot ring_slot(s, t)."""
        if self._frames is None:
            self._frames = np.stack([self.frame(s, t) for s in range(STREAMS) for t in range(TICKS)])
        return self._frames

    @staticmethod
    def ring_slot(stream, t):
        return stream * TICKS + t

    def aligned(self, stream, t, to_frame):
        """The float64 aligned face [OUT,OUT,3] of a warp whose inverse (aligned px -> frame px) is `to_frame`."""
        vv, uu = np.mgrid[0:OUT, 0:OUT].astype(f64)
        x = to_frame[0, 0] * uu + to_frame[0, 1] * vv + to_frame[0, 2]
        y = to_frame[1, 0] * uu + to_frame[1, 1] * vv + to_frame[1, 2]
        return self.scene(stream, t, x, y)

    def mesh_face(self, stream, t, mesh, lm, to_frame):
        """The float64 shape-normalised face: every aligned pixel is the scene at the barycentric blend of its
        triangle's frame vertices -- the landmarks `lm`, and the anchors placed by `to_frame`.  (A pixel on an edge that
        two triangles share gets the same point from either: the piecewise-affine map is continuous.)"""
        pts = np.asarray(mesh.points, f64)
        src = np.concatenate([np.asarray(lm, f64), apply(to_frame, pts[mesh.n_landmarks:])])
        vv, uu = np.mgrid[0:OUT, 0:OUT].astype(f64)
        x, y = np.full(uu.shape, np.nan), np.full(uu.shape, np.nan)
        for i, j, k in np.asarray(mesh.triangles):
            a, b, c = pts[i], pts[j], pts[k]
            det = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
            wb = ((uu - a[0]) * (c[1] - a[1]) - (vv - a[1]) * (c[0] - a[0])) / det
            wc = ((b[0] - a[0]) * (vv - a[1]) - (b[1] - a[1]) * (uu - a[0])) / det
            wa = 1.0 - wb - wc
            inside = (wa >= -1e-12) & (wb >= -1e-12) & (wc >= -1e-12) & np.isnan(x)
            x[inside] = (wa * src[i, 0] + wb * src[j, 0] + wc * src[k, 0])[inside]
            y[inside] = (wa * src[i, 1] + wb * src[j, 1] + wc * src[k, 1])[inside]
        assert not np.isnan(x).any()
        return self.scene(stream, t, x, y)

    # ---- the detector -----------------------------------------------------------------------------------------------------
    def detections(self, t):
        """Per stream, the integer boxes (x0,y0,x1,y1) of a detector at tick t, by ascending x0, and the faces they are of:
        the bounding box of the truth landmarks, 15 % of its longer side wider all round, of every face whose crop centre
        lies inside the frame."""
        boxes, who = [], []
        for s in range(STREAMS):
            found = []
            for f in self.faces:
                if f.stream != s or not f.rendered(t):
                    continue
                cx, cy = apply(f.pose(t), CENTRE[None])[0]
                if not (0.0 <= cx <= FW - 1 and 0.0 <= cy <= FH - 1):
                    continue
                lm = f.landmarks(t)
                pad = 0.15 * float((lm.max(0) - lm.min(0)).max())
                lo, hi = np.floor(lm.min(0) - pad).astype(int), np.ceil(lm.max(0) + pad).astype(int)
                found.append(([int(lo[0]), int(lo[1]), int(hi[0]), int(hi[1])], f))
            found.sort(key=lambda bf: bf[0][0])
            boxes.append([b for b, _ in found])
            who.append([f for _, f in found])
        return boxes, who

    def truth(self):
        """float64 [TICKS, CAP, 68, 2]: the truth landmarks of every slot at every tick, -1 where the slot holds no face."""
        out = np.full((TICKS, CAP, C, 2), -1.0)
        for t in range(TICKS):
            for f in self.faces:
                if f.live(t):
                    out[t, f.global_slot] = f.landmarks(t)
        return out

    def whole(self, f, t):
        """The face's aligned square, two frame px around it included, lies inside the frame at ticks t-1 and t: its crops
        then show no clamped edge, and the flow between the two ticks sees nothing but the face."""
        sq = np.array([[-0.5, -0.5], [OUT - 0.5, -0.5], [-0.5, OUT - 0.5], [OUT - 0.5, OUT - 0.5]])
        for tt in (t - 1, t):
            if tt < f.first:
                return False
            p = apply(f.pose(tt), sq)
            if p[:, 0].min() < 2 or p[:, 1].min() < 2 or p[:, 0].max() > FW - 3 or p[:, 1].max() > FH - 3:
                return False
        return True

    def step_bound(self):
        """The bound of a `step` tick's frame-space landmarks against truth, in frame px.  The truth goes through a float32
        crop matrix in float64 and comes back through the same matrix in float64.  Forward: two products and two sums per
        coordinate on values below 512, then the grid scale and its undoing: 6 roundings of at most half an ulp of 512,
        2^-44, in crop px.  The way back divides that by the crop scale s (crop px per frame px), and both crop
        coordinates feed each frame coordinate: a factor sqrt(2) / s; its own subtraction, two products, difference and
        division add 6 more roundings in frame px.  Doubled for what the roundings of the determinant and the
        second-order terms add."""
        s_min = min((IN - 1.0) / ((OUT - 1.0) * f.scale(t)) for f in self.faces for t in range(TICKS) if f.live(t))
        return 2.0 * 2.0 ** -44 * (6.0 * math.sqrt(2.0) / s_min + 6.0)

    def last_key(self, t):
        return t - t % KEY

    def flow_whole(self, f, t):
        """On a `step_flow` tick: the face has been whole at every tick since the last `step`.  The landmarks the flow
        carries over a clamped frame edge wander, and the aligned square fitted to them may leave the face's patch."""
        return all(self.whole(f, tt) for tt in range(self.last_key(t) + 1, t + 1))

    def flow_checked(self, f, t):
        """On a `step_flow` tick, the landmarks of face f whose carried position is held against truth (bool [68]), or
        None where none is.  The flow follows PIXELS, so it can follow truth only where the landmarks move with the
        pixels and the pixels keep their look:
          * the face is planar (the head's landmarks turn in 3-D over a texture that is moved by a similarity);
          * since the last `step` it has been whole at every tick: no crop showed a clamped frame edge;
          * since the last `step`, that tick included, its blur has been an ordinary one: a jump of the blur between two
            frames changes what the flow matches, and the points it then carries are off by a crop px and more (the
            schedule puts every jump on a `step` tick and the tick after it);
          * the landmark's 15 x 15 window lies inside the crop at every tick since the last `step`: the flow clamps its taps
            at the crop's border, so a window over the border (the jaw, the chin) matches replicated pixels."""
        k = self.last_key(t)
        if (self.is_key(t) or not isinstance(f, Planar) or not all(self.whole(f, tt) for tt in range(k + 1, t + 1))
                or any(tt in f.sharp for tt in range(k, t + 1))):
            return None
        inside = np.ones(C, bool)
        for tt in range(k + 1, t + 1):
            crop = matrix(umeyama(f.landmarks(tt - 1), CROP_TEMPLATE))       # the crop of tick tt: the fit of tick tt - 1
            for lm in (f.landmarks(tt - 1), f.landmarks(tt)):
                p = apply(crop, lm)
                inside &= (p.min(1) >= FLOW_RADIUS) & (p.max(1) <= IN - 1 - FLOW_RADIUS)
        return inside

    def eligible(self, f, t):
        """The ticks whose face may be taken as a best shot: the track is held and the step's status is 0."""
        return f.live(t) and not (t == f.last and t < TICKS - 1)

    def best_tick(self, f):
        """The scripted sharpest tick of a track: the one tick without blur."""
        (t,) = [t for t, s in f.sharp.items() if s == 0.0]
        return t

    def pose_bins(self, f, views):
        """tick -> pose bin of the truth landmarks under the package's HeadModel and `views` (an alignment.PoseViews), by
        tests/head_pose_ref.py and tests/track_views_ref.py."""
        import head_pose_ref
        import track_views_ref
        out = {}
        for t in range(TICKS):
            if self.eligible(f, t):
                rec = head_pose_ref.fit_one(f.landmarks(t), None, HEAD_INDICES, HEAD_POINTS)
                out[t] = track_views_ref.bin_of(rec, views.u_edges, views.v_edges)
        return out

    def view_ticks(self, f, views):
        """bin -> the scripted sharpest tick of the bin (the least blur among its ticks), for the bins the face visits."""
        out = {}
        for t, b in self.pose_bins(f, views).items():
            if b not in out or f.blur(t) < f.blur(out[b]):
                out[b] = t
        return out

    def track_ids(self):
        """face name -> track id: ids count up in the order the tracks begin, by ascending slot within a tick."""
        order = sorted(self.faces, key=lambda f: (f.first, f.global_slot))
        return {f.name: i for i, f in enumerate(order)}


class TruthSource:
    """A stand-in for the landmark model: `forward_device` returns the truth landmarks of the current tick on the output
    grid, through the tracker's current crop matrices, with torch ops on the device:
    grid = (M_crop . truth_frame) * (grid / in).  No host round trip.  For "landmark_stats" every record is
    (x, y) + SCORE_RECORD: a score of exactly 1, and other values in the columns a fit must not read."""
    n_classes, input_height, input_width, output_height, output_width = C, IN, IN, GRID, GRID
    max_batch = 1 << 20

    def __init__(self, script, device="cuda"):
        import torch
        self.truth = torch.from_numpy(script.truth()).to(device)
        self.tail = torch.tensor(SCORE_RECORD, dtype=torch.float64, device=device)
        self.tracker, self.tick, self.sent = None, 0, {}

    def bind(self, tracker):
        self.tracker = tracker

    def new_workspace(self, n, out="probs", n_points=0, opts=None):
        return None

    def forward_device(self, x, out="probs", n_points=0, thresh=0.0, out_tensor=None, workspace=None, opts=None):
        import torch
        if out not in ("landmarks", "landmark_stats"):
            raise ValueError("the truth source returns landmarks or landmark_stats (got %r)" % (out,))
        m = self.tracker.m_crop.to(torch.float64)
        p = self.truth[self.tick]
        if int(x.shape[0]) != int(p.shape[0]) or tuple(x.shape[1:]) != (IN, IN, 3):
            raise ValueError("the truth source serves `step`: one %dx%d crop per slot" % (IN, IN))
        px, py = p[..., 0], p[..., 1]
        cx = (m[:, 0, 0, None] * px + m[:, 0, 1, None] * py) + m[:, 0, 2, None]
        cy = (m[:, 1, 0, None] * px + m[:, 1, 1, None] * py) + m[:, 1, 2, None]
        empty = px < 0
        gx = torch.where(empty, px, cx * (GRID / IN))
        gy = torch.where(empty, py, cy * (GRID / IN))
        lm = torch.stack([gx, gy], -1)
        self.sent[self.tick] = lm
        if out == "landmarks":
            return lm
        return torch.cat([lm, self.tail.expand(lm.shape[0], lm.shape[1], 4)], -1)
