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

The row forms.  `step_active`, `step_live` and `step_flow_live` hand the model ROWS gathered from the slots, and which
slot a row serves is known only to the private snapshot of those calls.  `RowTruthSource` is `TruthSource` for them: bound
to a tracker it wraps that one instance's `_forward_landmarks`, notes the snapshot's "slot" and "m", and returns for every
row the truth of the row's slot through the row's own matrix ((-1,-1) for an inert row), in `TruthSource`'s order of
operations.  `SCHEDULES` names the three row schedules tests/test_gpu_scenario_rows.py runs, `RowsReference` is the loop of
the tracker's row calls on the numpy references (what stands in for the device in tests/test_scenario_host.py, and where
the landmark bound of a lagged crop comes from), and the `check_*` functions are the expectations both modules hold a run
to; each raises an AssertionError that begins with its own name.

What is left out: the pixels, poses, galleries and ids of a run are the device's alone -- `RowsReference` models the row map,
the step, the filter, the waits, the pending best-shot resets and the flow history, not the warps."""
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

    def truth(self, rendered=False):
        """float64 [TICKS, CAP, 68, 2]: the truth landmarks of every slot at every tick, -1 where the slot holds no face.
        rendered: a face stays in the table past its last tick, until the next face of its slot begins -- a schedule that
        serves a slot late sees the face the frame still shows (`occupant`)."""
        out = np.full((TICKS, CAP, C, 2), -1.0)
        for t in range(TICKS):
            for g in range(CAP):
                f = self.occupant(g, t) if rendered else self.face_in(g, t)
                if f is not None:
                    out[t, g] = f.landmarks(t)
        return out

    def occupant(self, slot, t):
        """The face the frames show for the global slot at tick t: the last one of the slot that has begun, or None."""
        began = [f for f in self.faces if f.global_slot == slot and f.first <= t]
        return max(began, key=lambda f: f.first) if began else None

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


class RowTruthSource(TruthSource):
    """`TruthSource` for the row forms.  `bind(tracker)` wraps that instance's `_forward_landmarks` in a closure that notes
    the `src` dict the step sequence hands it -- the snapshot of `step_active`, `step_live` and `step_flow_live`, which
    has a "slot" -- and calls the original; `forward_device` then returns, for row r, the truth of slot src["slot"][r]
    through src["m"][r], and (-1,-1) for an inert row (slot -1).  A `src` without "slot" is `step`'s: the call is
    `TruthSource`'s own.  The arithmetic is `TruthSource`'s, operation for operation, so a row of a full budget has the
    bits of the `step` row of its slot.  truth: None (Script.truth()) or another table of that shape.  `rows[tick]` keeps
    (slot, m, the landmarks sent, dt or None) of the last forward of a tick, on the device."""

    def __init__(self, script, device="cuda", truth=None):
        import torch
        super().__init__(script, device)
        if truth is not None:
            self.truth = torch.from_numpy(np.ascontiguousarray(truth, f64)).to(device)
        self.src, self.rows = None, {}

    def bind(self, tracker):
        self.tracker = tracker
        inner = tracker._forward_landmarks

        def noted(ring, src, workspace):
            self.src = src
            try:
                return inner(ring, src, workspace)
            finally:
                self.src = None

        tracker._forward_landmarks = noted

    def forward_device(self, x, out="probs", n_points=0, thresh=0.0, out_tensor=None, workspace=None, opts=None):
        import torch
        src = self.src
        if src is None or src.get("slot") is None:
            return super().forward_device(x, out, n_points, thresh, out_tensor, workspace, opts)
        if out not in ("landmarks", "landmark_stats"):
            raise ValueError("the truth source returns landmarks or landmark_stats (got %r)" % (out,))
        slot = src["slot"].to(torch.int64)
        m = src["m"].to(torch.float64)
        if int(x.shape[0]) != int(slot.shape[0]) or tuple(x.shape[1:]) != (IN, IN, 3):
            raise ValueError("the row truth source serves one %dx%d crop per row of the snapshot" % (IN, IN))
        inert = (slot < 0) | (slot >= self.truth.shape[1])
        p = torch.where(inert[:, None, None], self.truth.new_full((), -1.0), self.truth[self.tick][slot.clamp(0, self.truth.shape[1] - 1)])
        px, py = p[..., 0], p[..., 1]
        cx = (m[:, 0, 0, None] * px + m[:, 0, 1, None] * py) + m[:, 0, 2, None]
        cy = (m[:, 1, 0, None] * px + m[:, 1, 1, None] * py) + m[:, 1, 2, None]
        empty = px < 0
        gx = torch.where(empty, px, cx * (GRID / IN))
        gy = torch.where(empty, py, cy * (GRID / IN))
        lm = torch.stack([gx, gy], -1)
        self.sent[self.tick] = lm
        dt = src.get("dt")
        self.rows[self.tick] = (src["slot"].clone(), src["m"].clone(), lm, dt.clone() if isinstance(dt, torch.Tensor) else dt)
        if out == "landmarks":
            return lm
        return torch.cat([lm, self.tail.expand(lm.shape[0], lm.shape[1], 4)], -1)


def slots_truth(truth_t, m_crop):
    """`TruthSource.forward_device` in numpy: truth_t float64 [K,C,2] of one tick, m_crop float32 [K,2,3] -> the grid
    landmarks float64 [K,C,2]."""
    p = np.asarray(truth_t, f64)
    m = np.asarray(m_crop, np.float32).astype(f64)
    px, py = p[..., 0], p[..., 1]
    cx = (m[:, 0, 0, None] * px + m[:, 0, 1, None] * py) + m[:, 0, 2, None]
    cy = (m[:, 1, 0, None] * px + m[:, 1, 1, None] * py) + m[:, 1, 2, None]
    empty = px < 0
    return np.stack([np.where(empty, px, cx * (GRID / IN)), np.where(empty, py, cy * (GRID / IN))], -1)


def rows_truth(truth_t, slot, m_rows):
    """`RowTruthSource.forward_device` in numpy: the truth of every row's slot through the row's matrix; an inert row
    (a slot outside [0, K)) is (-1,-1)."""
    truth_t = np.asarray(truth_t, f64)
    slot = np.asarray(slot, np.int64)
    inert = (slot < 0) | (slot >= len(truth_t))
    p = np.where(inert[:, None, None], -1.0, truth_t[np.clip(slot, 0, len(truth_t) - 1)])
    return slots_truth(p, m_rows)


# ---- the row schedules ------------------------------------------------------------------------------------------------------
BUDGET = 3      # L-budget: three rows for the four faces that are live for most of the script


def schedule_full(t):
    """L-full: `step_live` on the detector's ticks, `step_flow_live` between, every stream, a budget of every slot."""
    return ("live" if t % KEY == 0 else "flow"), list(range(STREAMS)), CAP


def schedule_budget(t):
    """L-budget: `step_live` at every tick, every stream, BUDGET rows."""
    return "live", list(range(STREAMS)), BUDGET


def schedule_clock(t):
    """L-clock: `step_active`, stream 0 at every tick and stream 1 at every second one (the even ticks: the detector's
    ticks are among them)."""
    return "active", ([0, 1] if t % 2 == 0 else [0]), None


SCHEDULES = dict(full=schedule_full, budget=schedule_budget, clock=schedule_clock)
FAULTS = ("rows swapped", "wrong slot", "no wait", "reset unserved", "history kept")


def filter_dt():
    return alignment.LandmarkFilter().time_step(None)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint8).reshape(x.shape[0], -1) if x.ndim else x.view(np.uint8)


class RowsReference:
    """The loop of `update` + a row call per tick on the numpy references alone: tests/track_assoc_ref.py on the detector's
    ticks, then tests/track_live_ref.py, tests/flow_rows_ref.py (the flow gather and the history rule) or
    tests/track_rows_ref.py (the streams gather) for the snapshot, `rows_truth` -- or tests/flow_ref.py on crops of the
    rendered frames -- for the landmarks, and tests/track_rows_ref.py for the step.  It keeps what the tracker's host layer
    keeps around those calls: the cursors, `slot_age`, the pending best-shot resets and `flow_ready` / `flow_frame`.
    fault: None or one of FAULTS -- a tracker that is wrong in exactly that way, for tests/test_scenario_host.py.
    run() -> one record per tick, in the format of the `check_*` functions below."""

    def __init__(self, script, schedule, smooth=False, fault=None):
        assert fault is None or fault in FAULTS
        self.S, self.schedule, self.smooth, self.fault = script, schedule, smooth, fault
        self.truth = script.truth(rendered=True)

    def state(self):
        return {k: np.array(v, copy=True) for k, v in self.st.items() if v is not None}

    def update(self, t):
        import track_assoc_ref
        st = self.st
        det, _ = self.S.detections(t)
        before = st["m_crop"].copy()
        out = []
        for s in range(STREAMS):
            lo, hi = s * SLOTS, (s + 1) * SLOTS
            fs = None if not self.smooth else st["filter_state"][lo:hi]
            was_empty = np.array([track_assoc_ref.empty(track_assoc_ref.clip(b, FH, FW)) for b in st["boxes"][lo:hi]])
            r = track_assoc_ref.associate(np.asarray(det[s], np.int32).reshape(-1, 4), None, st["m_crop"][lo:hi],
                                          st["boxes"][lo:hi], st["status"][lo:hi], st["misses"][lo:hi], fs, IN, IN, FH, FW)
            for name in ("m_crop", "boxes", "status", "misses"):
                st[name][lo:hi] = r[name]
            if self.smooth:
                st["filter_state"][lo:hi] = r["state"]
            st["best_reset"][lo:hi][was_empty & (r["slot_det"] >= 0)] = 1
            out.append([int(v) + lo if v >= 0 else int(v) for v in r["det_slot"]])
        wrote = (_bits(st["m_crop"]) != _bits(before)).any(1)
        st["flow_ready"][wrote] = 0
        return out

    def gather(self, call, on, budget, frame_idx):
        import flow_rows_ref
        import track_live_ref
        import track_rows_ref
        st = self.st
        dt = filter_dt() if self.smooth else None
        mask = np.array([1 if s in on else 0 for s in range(STREAMS)], np.int32)
        on_slot = np.repeat(mask != 0, SLOTS)
        if call == "active":
            assert not self.smooth
            g = track_rows_ref.gather_streams(on, STREAMS, SLOTS, st["m_crop"], st["boxes"], frame_idx, None, None, st["best_reset"])
            snap = dict(slot=g["slot"], m=g["m"], boxes=g["boxes"], frame_index=g["frame_index"], reset=g["reset"], dt=None,
                        counts=None)
            st["best_reset"] = g["reset_global"]
            st["flow_ready"][on_slot] = 0
        elif call == "live":
            g = track_live_ref.gather_live(st["m_crop"], st["boxes"], STREAMS, SLOTS, FH, FW, budget, mask, frame_idx, None, dt,
                                           None, st["best_reset"], st["slot_age"] if self.smooth else None, int(st["live_cursor"][0]))
            snap = dict(slot=g["slot"], m=g["m"], boxes=g["boxes"], frame_index=g["frame_index"], reset=g["reset"], dt=g["dt"],
                        counts=g["counts"])
            st["best_reset"] = g["reset_global"]
            st["live_cursor"][0] = g["cursor_global"]
            if self.smooth:
                st["slot_age"] = g["age_global"]
            if self.fault == "history kept":      # the history is cleared for the rows alone, not for the stepped streams
                st["flow_ready"][g["slot"][g["slot"] >= 0]] = 0
            else:
                st["flow_ready"][on_slot] = 0
        else:
            g = flow_rows_ref.gather_flow(dict(s=STREAMS, k=SLOTS, fh=FH, fw=FW, n=budget, dt=dt, stream_on=mask,
                                               frame_idx_stream=frame_idx, reset=st["best_reset"],
                                               age=st["slot_age"] if self.smooth else None, cursor=st["flow_cursor"],
                                               m_crop=st["m_crop"], boxes=st["boxes"], flow_frame=st["flow_frame"],
                                               flow_ready=st["flow_ready"]))
            snap = dict(slot=g["slot_c"], m=g["m_c"], boxes=g["boxes_c"], frame_index=g["frame_idx_c"],
                        prev_frame_index=g["prev_frame_idx_c"], reset=g["reset_c"], dt=g.get("dt_c"), counts=g["counts"])
            st["best_reset"], st["flow_cursor"], st["flow_ready"] = g["reset"], g["cursor"], g["flow_ready"]
            if self.smooth:
                st["slot_age"] = g["age"]
        served = snap["slot"][snap["slot"] >= 0]
        if self.fault == "reset unserved" and call != "active":   # the pending resets of every live slot are used up
            for s in range(STREAMS * SLOTS):
                if on_slot[s] and not track_live_ref.box_empty(st["boxes"][s], FH, FW):
                    st["best_reset"][s] = 0
        if self.fault == "rows swapped" and len(served) >= 2:     # the map alone: matrices and boxes stay where they were
            snap["slot"] = snap["slot"].copy()
            snap["slot"][[0, 1]] = snap["slot"][[1, 0]]
        if self.fault == "no wait" and snap["dt"] is not None:
            snap["dt"] = np.where(snap["slot"] >= 0, dt, snap["dt"])
        return snap

    def flow_landmarks(self, snap):
        import flow_ref
        import mesh_ref
        frames = self.S.frames()
        n = len(snap["slot"])
        lm, w, flags = np.full((n, C, 2), -1.0), np.zeros((n, C)), np.ones((n, C), np.int32)
        for r, g in enumerate(snap["slot"]):
            if g < 0:
                continue
            crop = lambda i: np.clip(np.rint(mesh_ref.warp_affine_frame_ref(frames[i], snap["m"][r], IN, IN)), 0, 255).astype(np.uint8)
            fl = flow_ref.landmark_flow(crop(snap["prev_frame_index"][r])[None], crop(snap["frame_index"][r])[None],
                                        self.st["hist_lm"][g][None], snap["m"][r][None], flow_ref.options())
            lm[r], w[r], flags[r] = fl[0][0], fl[1][0], fl[3][0]
        return lm, w, flags

    def run(self):
        import flow_rows_ref
        import track_filter_ref
        import track_ref
        import track_rows_ref
        k = CAP
        self.st = st = dict(
            m_crop=np.broadcast_to(track_ref.IDENTITY, (k, 2, 3)).copy(), boxes=np.zeros((k, 4), np.int32),
            status=np.full(k, track_ref.DEAD, np.int32), misses=np.zeros(k, np.int32), best_reset=np.zeros(k, np.int32),
            flow_ready=np.zeros(k, np.int32), flow_frame=np.zeros(k, np.int32), live_cursor=np.zeros(1, np.int32),
            flow_cursor=np.zeros(1, np.int32), hist_lm=np.full((k, C, 2), -1.0),
            filter_state=track_filter_ref.empty_state(k, C) if self.smooth else None,
            slot_age=np.zeros(k) if self.smooth else None)
        filt = dict(track_filter_ref.DEFAULTS) if self.smooth else None
        out = []
        for t in range(TICKS):
            call, on, budget = self.schedule(t)
            rec = dict(t=t, call=call, on=list(on), budget=budget)
            if self.S.is_key(t):
                rec["det_slot"] = self.update(t)
            rec["pre"] = self.state()
            frame_idx = np.array([self.S.ring_slot(s, t) for s in range(STREAMS)], np.int32)
            snap = self.gather(call, on, budget, frame_idx)
            if call == "flow":
                lm, w, rec["flags"] = self.flow_landmarks(snap)
                scale = 1.0
            else:
                lm, w, scale = rows_truth(self.truth[t], snap["slot"], snap["m"]), np.ones((len(snap["slot"]), C)), IN / GRID
            write = snap["slot"]
            if self.fault == "wrong slot" and (write >= 0).sum() >= 2:      # the rows land one served slot further on
                write = write.copy()
                write[write >= 0] = np.roll(write[write >= 0], 1)
            r = track_rows_ref.step_rows(lm, w, snap["m"], snap["boxes"], write, scale, scale, IN, IN, FH, FW, CROP_TEMPLATE,
                                         TEMPLATE, st["m_crop"], st["boxes"], st["status"], st["filter_state"], snap["dt"], filt)
            st["m_crop"], st["boxes"], st["status"] = r["m_next"], r["boxes_next"], r["status"]
            if self.smooth:
                st["filter_state"] = r["state"]
            raw = r["lm_raw"] if self.smooth else r["lm_frame"]
            st["hist_lm"], _, st["flow_frame"], st["flow_ready"] = flow_rows_ref.history_put(
                write, r["status_rows"], snap["frame_index"], st["flow_frame"], st["flow_ready"], raw, st["hist_lm"])
            rec.update(slot=snap["slot"], counts=snap["counts"], m_c=snap["m"], boxes_c=snap["boxes"], dt_c=snap["dt"], sent=lm,
                       w=w, lm=r["lm_frame"], M=r["m_align"], status_rows=r["status_rows"], post=self.state())
            out.append(rec)
        return out


# ---- what a run of a row schedule is held to ------------------------------------------------------------------------------
RETIRE_NAMES = ("track_id", "born_frame", "_born", "_exit_stale")     # the per-slot state the retire call owns
NOT_PER_SLOT = ("exit_row",)                                         # rewritten for every slot by every retire call


def served(rec):
    """row -> slot of the rows that serve one."""
    return {r: int(g) for r, g in enumerate(rec["slot"]) if g >= 0}


def on_slots(rec):
    return [g for g in range(CAP) if g // SLOTS in rec["on"]]


def live_before(rec):
    import track_live_ref
    return [g for g in on_slots(rec) if not track_live_ref.box_empty(rec["pre"]["boxes"][g], FH, FW)]


def check_row_map(rec):
    """The rows of a tick are the numpy gather of the state before it: tests/track_live_ref.py for `step_live`,
    tests/flow_rows_ref.py for `step_flow_live`, tests/track_rows_ref.py for `step_active`; the counts and the cursor too."""
    import flow_rows_ref
    import track_live_ref
    import track_rows_ref
    pre, post, t = rec["pre"], rec["post"], rec["t"]
    mask = np.array([1 if s in rec["on"] else 0 for s in range(STREAMS)], np.int32)
    if rec["call"] == "active":
        want = track_rows_ref.gather_streams(rec["on"], STREAMS, SLOTS, pre["m_crop"], pre["boxes"])["slot"]
        counts = cursor = None
    elif rec["call"] == "live":
        g = track_live_ref.gather_live(pre["m_crop"], pre["boxes"], STREAMS, SLOTS, FH, FW, rec["budget"], mask,
                                       cursor=int(pre["live_cursor"][0]))
        want, counts, cursor = g["slot"], g["counts"], ("live_cursor", g["cursor_global"])
    else:
        g = flow_rows_ref.gather_flow(dict(s=STREAMS, k=SLOTS, fh=FH, fw=FW, n=rec["budget"], dt=None, stream_on=mask,
                                           cursor=pre["flow_cursor"], m_crop=pre["m_crop"], boxes=pre["boxes"],
                                           flow_frame=pre["flow_frame"], flow_ready=pre["flow_ready"]))
        want, counts, cursor = g["slot_c"], g["counts"], ("flow_cursor", int(g["cursor"][0]))
    assert np.array_equal(rec["slot"], want), "check_row_map: tick %d rows serve slots %s, the reference gathers %s" % (
        t, rec["slot"].tolist(), want.tolist())
    if counts is not None:
        assert np.array_equal(rec["counts"], counts), "check_row_map: tick %d counts %s, reference %s" % (t, rec["counts"], counts)
        assert int(post[cursor[0]][0]) == int(cursor[1]), "check_row_map: tick %d %s" % (t, cursor[0])
    for r, g in served(rec).items():
        for name, src in (("m_c", "m_crop"), ("boxes_c", "boxes")):
            if name in rec:
                assert _bits(rec[name][r:r + 1]).tobytes() == _bits(pre[src][g:g + 1]).tobytes(), \
                    "check_row_map: tick %d row %d does not carry the %s of slot %d" % (t, r, src, g)


def check_untouched(rec):
    """A slot that is no row of the tick keeps every bit of its per-slot state.  Three kinds of state have rules of their
    own and are held elsewhere: `flow_ready` of a stepped stream (check_flow_ready), `slot_age` of a stepped stream
    (check_smoothing), and what the retire call owns (RETIRE_NAMES) at a slot where that call has work -- a birth to
    name, or an emptied slot whose track it queues; it runs over all slots whichever of them the tick serves."""
    import track_live_ref
    pre, post, t = rec["pre"], rec["post"], rec["t"]
    rows, on = set(served(rec).values()), set(on_slots(rec))
    for name, a in pre.items():
        if a.ndim == 0 or a.shape[0] != CAP or name in NOT_PER_SLOT:
            continue
        b = post[name]
        for g in range(CAP):
            if g in rows or (name in ("flow_ready", "slot_age") and g in on):
                continue
            if name in RETIRE_NAMES and (pre["_born"][g] != 0 or (
                    pre["track_id"][g] >= 0 and track_live_ref.box_empty(pre["boxes"][g], FH, FW))):
                continue
            assert _bits(a[g:g + 1]).tobytes() == _bits(b[g:g + 1]).tobytes(), \
                "check_untouched: tick %d changed %s of slot %d, which it did not serve" % (t, name, g)


def check_flow_ready(rec):
    """The history rule: after a tick, a slot of a stepped stream has a usable history exactly when the tick served it with
    status 0 -- a live slot the budget left out has none --, and a slot of any other stream keeps what it had."""
    pre, post, t = rec["pre"], rec["post"], rec["t"]
    if "flow_ready" not in pre:
        return
    alive = {g for r, g in served(rec).items() if rec["status_rows"][r] == 0}
    on = set(on_slots(rec))
    for g in range(CAP):
        want = int(g in alive) if g in on else int(pre["flow_ready"][g])
        assert int(post["flow_ready"][g]) == want, "check_flow_ready: tick %d slot %d has flow_ready %d, the rule says %d" % (
            t, g, int(post["flow_ready"][g]), want)


def check_rows_written(rec):
    """What a row returned is what its OWN slot holds afterwards: the status, and the next crop's matrix -- the float32
    fit of the row's landmarks to the crop template (tests/track_ref.py, whose bits the step has), the identity for a row
    that lost its track."""
    import track_ref
    post, t = rec["post"], rec["t"]
    for r, g in served(rec).items():
        st = int(rec["status_rows"][r])
        assert int(post["status"][g]) == st, "check_rows_written: tick %d row %d returned status %d, slot %d holds %d" % (
            t, r, st, g, int(post["status"][g]))
        want = track_ref.IDENTITY if st else track_ref.fit(rec["lm"][r], rec["w"][r] if "w" in rec else None, CROP_TEMPLATE)[0]
        assert _bits(post["m_crop"][g:g + 1]).tobytes() == _bits(want[None]).tobytes(), \
            "check_rows_written: tick %d slot %d does not hold the fit of row %d's landmarks" % (t, g, r)


def check_rotation(records):
    """Every live slot of a stepped stream is served within ceil(live / budget) ticks.  -> (the longest wait in ticks, the
    rows served per tick)."""
    waited, longest, per_tick = np.zeros(CAP, int), 0, []
    for rec in records:
        live, rows = live_before(rec), set(served(rec).values())
        allowed = -(-len(live) // rec["budget"]) if live else 1
        per_tick.append(len(rows))
        for g in range(CAP):
            waited[g] = waited[g] + 1 if (g in live and g not in rows) else 0
            longest = max(longest, int(waited[g]))
            assert waited[g] < allowed, "check_rotation: tick %d slot %d has waited %d ticks with %d live slots and a budget of %d" % (
                rec["t"], g, waited[g], len(live), rec["budget"])
        assert len(rows) == min(len(live), rec["budget"]), "check_rotation: tick %d served %d of %d live slots" % (
            rec["t"], len(rows), len(live))
    return longest, per_tick


def check_smoothing(S, records):
    """A tracker that smooths returns the landmarks of tests/track_filter_ref.py bit for bit, the reference driven by the
    landmarks the model was sent, by its own state in closed loop, and by each slot's OWN dt: the filter's time step plus
    the time the slot has waited unserved (tests/track_live_ref.py's `age`, restated from the rows of the earlier ticks).
    -> the number of coordinates the filter moved."""
    import track_filter_ref
    import track_live_ref
    import track_rows_ref
    dt = filter_dt()
    state, age, moved = track_filter_ref.empty_state(CAP, C), np.zeros(CAP), 0
    filt = dict(track_filter_ref.DEFAULTS)
    for rec in records:
        t, pre, post = rec["t"], rec["pre"], rec["post"]
        assert rec["call"] == "live"
        for f in S.faces:
            if f.first == t:                                            # a birth clears the slot's history
                state[f.global_slot] = -1.0
        mask = np.array([1 if s in rec["on"] else 0 for s in range(STREAMS)], np.int32)
        g = track_live_ref.gather_live(pre["m_crop"], pre["boxes"], STREAMS, SLOTS, FH, FW, rec["budget"], mask, dt=dt, age=age,
                                       cursor=int(pre["live_cursor"][0]))
        age = g["age_global"]
        r = track_rows_ref.step_rows(rec["sent"], rec["w"], rec["m_c"], rec["boxes_c"], g["slot"], IN / GRID, IN / GRID, IN, IN,
                                     FH, FW, CROP_TEMPLATE, TEMPLATE, pre["m_crop"], pre["boxes"], pre["status"], state, g["dt"], filt)
        state = r["state"]
        for name, got, want in (("landmarks", rec["lm"], r["lm_frame"]), ("M", rec["M"], r["m_align"]),
                                ("status", rec["status_rows"], r["status_rows"]), ("m_crop", post["m_crop"], r["m_next"]),
                                ("slot_age", post["slot_age"], age), ("filter_state", post["filter_state"], state)):
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), \
                "check_smoothing: tick %d %s is not the filter reference's under each slot's own dt (rows %s, dt %s)" % (
                    t, name, g["slot"].tolist(), g["dt"].tolist())
        moved += int((r["lm_frame"] != r["lm_raw"]).sum())
    return moved


def fit_bound(sim, pts):
    """The float32 rounding of the four numbers of a similarity, on the points it is applied to: per coordinate
    2^-24 (|a| |x| + |b| |y| + |t|), and 1e-9 for the float64 arithmetic on either side."""
    a, b, tx, ty = [abs(v) for v in sim]
    x, y = np.abs(pts[:, 0]), np.abs(pts[:, 1])
    return 2.0 ** -24 * np.stack([a * x + b * y + tx, b * x + a * y + ty], 1) + 1e-9


def pose_tol(bound):
    """The head's angles on landmarks within `bound` frame px of truth (the host module holds the reference's angles on
    the truth itself within 1e-12 of the script).  The pose is read off the affine fit of the six centred model points:
    a change d of every image point changes its rows I, J by at most sqrt(6) d / sigma_min of the centred model matrix,
    their directions by that over the scale |I| = |J|, and each angle by at most the sum over the two rows; doubled for
    the arc functions away from the identity (|angles| < 40 degrees)."""
    x = HEAD_POINTS - HEAD_POINTS.mean(0)
    sigma = np.linalg.svd(x, compute_uv=False).min()
    scale = 0.1003 * 0.97
    return 1e-12 + 2.0 * 2.0 * math.sqrt(6.0) * bound / (sigma * scale)


def lagged_bound(m_c, truth_pts):
    """Script.step_bound() for ONE row whose crop may be some ticks old: the same count of roundings, with the crop scale
    s read off the crop matrix the row was cut with (m_c: the REFERENCE's float32 matrix, computed on the CPU) where
    step_bound() takes the smallest scale of the script, and with half an ulp of the row's own largest value where
    step_bound() writes 2^-44 for values below 512 -- never less than that; a face leaving through the right edge has
    landmarks beyond x = 512.  The truth must lie in the crop's positive quadrant (a negative point is a rejected one)."""
    m = np.asarray(m_c, np.float32).astype(f64)
    s = math.hypot(m[0, 0], m[1, 0])
    crop = apply(m, truth_pts)
    assert crop.min() >= 0.0, "lagged_bound: the truth leaves the crop's positive quadrant (%.2f)" % crop.min()
    top = max(float(np.abs(crop).max()), float(np.abs(truth_pts).max()), 511.0)
    half_ulp = 2.0 ** (math.floor(math.log2(top)) - 52 - 1)
    return 2.0 * half_ulp * (6.0 * math.sqrt(2.0) / s + 6.0)


def expected_status(S, f, t):
    """A served face is kept (0) until its scripted exit and dropped there, or at its first later serving, with
    TRACK_OUTSIDE."""
    return 16 if (t >= f.last and f.last < TICKS - 1) else 0


def check_truth(S, rec, ref, worst, mesh=None, ids=None):
    """A forward tick of a row call against the rendered truth, row by row: the expectations tests/test_gpu_scenario.py
    has for a `step` tick.  ref: the record of the same tick of `RowsReference` on the same schedule -- its crop matrices
    give the landmark bound of every row (`lagged_bound`).  worst: a dict of running maxima, updated.  What a record
    does not hold (aligned, mesh, pose, track_id: the reference has none of them) is not looked at.  A truth point left
    of, or above, a crop that is two ticks old has a negative crop coordinate, which the step rejects: the reference says
    which points those are (check_lifetimes holds them clear of zero), they must come back as (-1,-1) and no other may, and
    the bound, the fits and the mesh are those of the points that remain, as in tests/test_gpu_scenario.py."""
    t, post = rec["t"], rec["post"]
    truth = S.truth(rendered=True)[t]
    assert np.array_equal(ref["slot"], rec["slot"]), "check_truth: tick %d rows %s, reference %s" % (t, rec["slot"], ref["slot"])
    for r in range(len(rec["slot"])):
        g = int(rec["slot"][r])
        f = S.occupant(g, t) if g >= 0 else None
        st = int(rec["status_rows"][r])
        if g < 0 or ref["status_rows"][r] & 1:                     # an inert row, or the empty slot of an active stream
            assert st & 1 and (rec["lm"][r] == -1.0).all(), "check_truth: tick %d row %d of no face" % (t, r)
            for name in ("aligned", "mesh"):
                assert name not in rec or not rec[name][r].any(), "check_truth: tick %d row %d %s of no face" % (t, r, name)
            continue
        assert f is not None and st == expected_status(S, f, t), "check_truth: tick %d slot %d status %d" % (t, g, st)
        lm, tru = rec["lm"][r], truth[g]
        ok = ~(ref["sent"][r] < 0).any(1)        # the reference says which truth points lie outside the lagged crop
        assert (lm[~ok] == -1.0).all() and (lm[ok] >= 0).all(), "check_truth: tick %d %s rejects other landmarks than %s" % (
            t, f.name, list(np.flatnonzero(~ok)))
        bound = lagged_bound(ref["m_c"][r], tru[ok])
        e = float(np.abs(lm - tru)[ok].max())
        worst["lm"] = max(worst.get("lm", 0.0), e / bound)
        worst["lm_px"], worst["lm_bound"] = max(worst.get("lm_px", 0.0), e), max(worst.get("lm_bound", 0.0), bound)
        assert e <= bound, "check_truth: tick %d %s landmarks %.3e px from truth, bound %.3e" % (t, f.name, e, bound)
        for name, got, tmpl in (("M", rec["M"][r], TEMPLATE), ("m_next", post["m_crop"][g], CROP_TEMPLATE)):
            if name == "m_next" and st:
                assert np.array_equal(got, np.array([[1, 0, 0], [0, 1, 0]], np.float32)), "check_truth: tick %d %s" % (t, f.name)
                continue
            sim = umeyama(lm[ok], tmpl[ok])
            d = np.abs(apply(got, tru) - apply(matrix(sim), tru)) / fit_bound(sim, tru)
            if isinstance(f, Planar):
                d = np.maximum(d, np.abs(apply(got, tru) - tmpl) / fit_bound(sim, tru))
            worst["fit"] = max(worst.get("fit", 0.0), float(d.max()))
            assert d.max() <= 1.0, "check_truth: tick %d %s %s is %.3f of the float32 bound" % (t, f.name, name, float(d.max()))
        pix = b_align(f.blur(t), f.scale(t))
        if "aligned" in rec:
            e = float(np.abs(rec["aligned"][r] - S.aligned(f.stream, t, f.pose(t))).max()) / pix
            worst["aligned"] = max(worst.get("aligned", 0.0), e)
            assert e <= 1.0, "check_truth: tick %d %s aligned pixel at %.3f of B_align" % (t, f.name, e)
        if "mesh" in rec and ok.all():
            e = float(np.abs(rec["mesh"][r] - S.mesh_face(f.stream, t, mesh, tru, f.pose(t))).max()) / pix
            worst["mesh"] = max(worst.get("mesh", 0.0), e)
            assert e <= 1.0, "check_truth: tick %d %s mesh pixel at %.3f of B_align" % (t, f.name, e)
        if "pose" in post:
            pose = post["pose"][g]
            assert pose[14] == 1.0, "check_truth: tick %d %s pose not ok" % (t, f.name)
            if isinstance(f, Head):
                e, tol = float(np.abs(pose[15:18] - np.array(f.angles(t))).max()), pose_tol(bound)
                worst["pose"], worst["pose_tol"] = max(worst.get("pose", 0.0), e), max(worst.get("pose_tol", 0.0), tol)
                assert e <= tol, "check_truth: tick %d head pose %.3e rad from the script, bound %.3e" % (t, e, tol)
        if ids is not None and "track_id" in post:
            assert post["track_id"][g] == ids[f.name], "check_truth: tick %d %s has track id %d" % (t, f.name, post["track_id"][g])


def check_lifetimes(S, records):
    """The reference-alone condition of a schedule: every face is served from its first tick on, keeps its track (status
    0) at every serving up to its scripted exit, only the face that leaves is dropped, once, with TRACK_OUTSIDE, no row
    ever serves a slot without a face, and every detection goes to its face's slot.  -> name -> the ticks that served it."""
    seen, dropped = {f.name: [] for f in S.faces}, []
    for rec in records:
        t = rec["t"]
        if "det_slot" in rec:
            _, who = S.detections(t)
            assert rec["det_slot"] == [[f.global_slot for f in row] for row in who], "check_lifetimes: tick %d detections %s" % (
                t, rec["det_slot"])
        for r, g in served(rec).items():
            st = int(rec["status_rows"][r])
            if st & 1:
                assert rec["call"] == "active", "check_lifetimes: tick %d row %d serves the dead slot %d" % (t, r, g)
                continue
            f = S.occupant(g, t)
            assert f is not None and st == expected_status(S, f, t), "check_lifetimes: tick %d slot %d status %d" % (t, g, st)
            if rec["call"] != "flow":       # which truth points a lagged crop rejects must not hang on a rounding
                assert np.abs(rec["sent"][r]).min() > 1e-6 and (rec["lm"][r] < 0).all(1).sum() <= 4, \
                    "check_lifetimes: tick %d slot %d landmarks at the crop's edge" % (t, g)
                assert ((rec["lm"][r] < 0).all(1) == (rec["sent"][r] < 0).any(1)).all(), "check_lifetimes: tick %d slot %d" % (t, g)
            seen[f.name].append(t)
            if st:
                dropped.append(f.name)
    gone = [f.name for f in S.faces if f.last < TICKS - 1]
    assert dropped == gone, "check_lifetimes: dropped %s, the script drops %s" % (dropped, gone)
    for f in S.faces:
        assert seen[f.name] and seen[f.name][-1] >= min(f.last, TICKS - 2), "check_lifetimes: %s served at %s" % (f.name, seen[f.name])
    return seen
