"""NumPy restatement of the two wide camera models (checker only): vk::cameras::EquidistantDistortion (Kannala-Brandt,
src/vikit/vikit_cameras/include/vikit/cameras/equidistant_distortion.h:37-121) and vk::cameras::AtanDistortion (the FOV
model, atan_distortion.h).  Scalar maths through `math` (libm), not NumPy's vectorised atan / tan, so that a value stays
within an ulp or so of the device's ocml.

CamWide subclasses np_restatement_direct.Cam: the matcher, seed, stereo and candidate restatements take any camera with
distort / distort_jacobian / undistort / project3 / project3_jacobian / back_project3, so they run unchanged on it."""
import math

import numpy as np

from np_restatement_direct import Cam

NONE, RADTAN, EQUIDISTANT, ATAN = 0, 1, 2, 3
K_R_THRESH = 1e-8   # EquidistantDistortion::kRThresh


class EquidistantDistortion(object):
    def __init__(self, k1, k2, k3, k4):
        self.k1, self.k2, self.k3, self.k4 = float(k1), float(k2), float(k3), float(k4)

    def thetad_from_theta(self, theta):
        theta2 = theta * theta
        theta4 = theta2 * theta2
        theta6 = theta4 * theta2
        theta8 = theta4 * theta4
        return theta * (1.0 + self.k1 * theta2 + self.k2 * theta4 + self.k3 * theta6 + self.k4 * theta8)

    def deriv_thetad_from_theta(self, theta):
        theta2 = theta * theta
        theta4 = theta2 * theta2
        theta6 = theta4 * theta2
        theta8 = theta4 * theta4
        return 1 + 3 * self.k1 * theta2 + 5 * self.k2 * theta4 + 7 * self.k3 * theta6 + 9 * self.k4 * theta8

    def distort(self, x, y):
        r = math.sqrt(x * x + y * y)
        if r < K_R_THRESH:
            return x, y
        theta = math.atan(r)
        scaling = self.thetad_from_theta(theta) / r
        return x * scaling, y * scaling

    def jacobian(self, x, y):
        r = math.sqrt(x * x + y * y)
        if r < K_R_THRESH:
            return np.eye(2)
        inv_r = 1.0 / r
        r2 = r * r
        dr_du = x * inv_r
        dr_dv = y * inv_r
        theta = math.atan(r)
        dtheta_dr = 1.0 / (1 + r * r)
        thetad = self.thetad_from_theta(theta)
        dthetad_dr = self.deriv_thetad_from_theta(theta) * dtheta_dr
        scaling = thetad / r
        dscaling_du = (dthetad_dr * dr_du * r - dr_du * thetad) / r2
        dscaling_dv = (dthetad_dr * dr_dv * r - dr_dv * thetad) / r2
        return np.array([[dscaling_du * x + scaling, dscaling_dv * x],
                         [dscaling_du * y, dscaling_dv * y + scaling]])

    def undistort(self, x, y, iterations=5):
        """The reference's five fixed-point iterations (more for rendering: `iterations`).  thetad == 0 gives
        tan(0) / 0 = NaN, as in the reference."""
        thetad = math.sqrt(x * x + y * y)
        theta = thetad
        for _ in range(iterations):
            theta2 = theta * theta
            theta4 = theta2 * theta2
            theta6 = theta4 * theta2
            theta8 = theta4 * theta4
            theta = thetad / (1.0 + self.k1 * theta2 + self.k2 * theta4 + self.k3 * theta6 + self.k4 * theta8)
        scaling = math.tan(theta) / thetad if thetad != 0.0 else float("nan")
        return x * scaling, y * scaling


class AtanDistortion(object):
    def __init__(self, s):
        # initializeParameters
        self.s = float(s)
        self.s_inv = 1.0 / self.s
        self.tans = 2.0 * math.tan(self.s / 2.0)
        self.tans_inv = 1.0 / self.tans

    def distort(self, x, y):
        r = math.sqrt(x * x + y * y)
        factor = 1.0 if r < 0.001 else self.s_inv * math.atan(r * self.tans) / r
        return x * factor, y * factor

    def jacobian(self, x, y):
        raise NotImplementedError("AtanDistortion::jacobian is not implemented in the reference")

    def undistort(self, x, y, iterations=None):   # closed form: `iterations` is accepted for a common signature
        dist_r = math.sqrt(x * x + y * y)
        r = math.tan(dist_r * self.s) * self.tans_inv
        d_factor = r / dist_r if dist_r > 0.01 else 1.0
        return x * d_factor, y * d_factor


class CamWide(Cam):
    """A pinhole camera of any of the four models (model: NONE / RADTAN / EQUIDISTANT / ATAN; d: its parameters).
    dist stays what Cam reads for radtan, so the base class handles NONE and RADTAN unchanged."""

    def __init__(self, width, height, fx, fy, cx, cy, model=NONE, d=None):
        super(CamWide, self).__init__(width, height, fx, fy, cx, cy, d if model == RADTAN else None)
        self.model = int(model)
        self.d = None if d is None else [float(v) for v in d]
        if self.model == EQUIDISTANT:
            self.wide = EquidistantDistortion(*self.d[:4])
        elif self.model == ATAN:
            self.wide = AtanDistortion(self.d[0])
        else:
            self.wide = None

    @staticmethod
    def of(c):
        """From a synth.Camera (model / dist) or another CamWide."""
        model = getattr(c, "model", None)
        if model is None:
            model = NONE if c.dist is None else RADTAN
        model = {"none": NONE, "radtan": RADTAN, "equidistant": EQUIDISTANT, "atan": ATAN}.get(model, model)
        d = getattr(c, "d", None) if isinstance(c, CamWide) else c.dist
        return CamWide(c.width, c.height, c.fx, c.fy, c.cx, c.cy, model, d)

    def distort(self, x, y):
        return self.wide.distort(x, y) if self.wide else Cam.distort(self, x, y)

    def distort_jacobian(self, x, y):
        return self.wide.jacobian(x, y) if self.wide else Cam.distort_jacobian(self, x, y)

    def undistort(self, x, y):
        return self.wide.undistort(x, y) if self.wide else Cam.undistort(self, x, y)

    def project3_jacobian(self, p):
        # the device's order: J = diag(fx, fy) * (J_dist * d(uv)/d(xyz)), entry by entry
        z_inv = 1.0 / p[2]
        Jd = self.distort_jacobian(p[0] * z_inv, p[1] * z_inv)
        d = (z_inv, 0.0, -p[0] * z_inv * z_inv, 0.0, z_inv, -p[1] * z_inv * z_inv)
        J = np.zeros((2, 3))
        for k in range(3):
            J[0, k] = self.fx * (Jd[0, 0] * d[k] + Jd[0, 1] * d[3 + k])
            J[1, k] = self.fy * (Jd[1, 0] * d[k] + Jd[1, 1] * d[3 + k])
        return J
