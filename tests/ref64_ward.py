"""A binary64 restatement of the Ward BSDF (three model types) and of the Composite BSDF: f, pdf and sample(bRec, pdf, s),
written from src/bsdfs/ward.cpp, src/bsdfs/composite.cpp and include/mitsuba/core/pdf.h of the reference, not from csrc/.
It continues tests/ref64.py (same conventions: float32 inputs promoted to float64, every value with a conditioning factor
`cond` and a flag `amb` where float32 cannot decide a branch) and uses its helpers and its restatements of the other
plugins for a composite's children.  Test infrastructure.

A composite needs the table its child indices point into, so the three entry points live on `Table`; `Table.f / pdf /
sample` have the signatures of ref64.f / pdf / sample and fall through to them for types 0-7, so a Table can stand in for the
ref64 module wherever a check takes one (closed_forms.check_model, closed_forms.check_render).

Parameter blocks (include/mtsgpu.h):
  ward       [0] model type (0 ward, 1 ward-duer, 2 balanced) [1] alphaX [2] alphaY [3] kd [4] ks [5] specularSamplingWeight
             [6] diffuseSamplingWeight [7..9] diffuseReflectance [10..12] specularReflectance   (after Ward::configure)
  composite  [0] n [1..n] weights [1+n..2n] child indices into the table, as floats"""
import numpy as np

import ref64
from ref64 import (DIFFUSE_REFL, DIR_REACH, EPS32, GLOSSY_REFL, MARGIN, TWOSIDED, Sample, _dot, _f64, _mix_cond, _normalize,
                   _relevant, _rgb, square_to_hemisphere_psa)

WARD, COMPOSITE = 8, 9
SPEC_CUT = 1e-10                 # ward.cpp:180


def _ward_exponent(P, H):
    """ward.cpp:174-175 == :194-196: -((H.x / alphaX)^2 + (H.y / alphaY)^2) / H.z^2, the same for H and any multiple of it"""
    f2, f3 = H[:, 0] / P[1], H[:, 1] / P[2]
    return -(f2 * f2 + f3 * f3) / (H[:, 2] * H[:, 2])


def ward_f(P, wi, wo):
    """Ward::f (ward.cpp:142-188), typeMask = EAll, component = -1 -> (value [n][3], cond, amb).
    The exponent carries the rounding of H = wi + wo and of the two quotients (about 6 eps relative), which exp()
    turns into 6 |exponent| eps of the value.  The branch `specRef > 1e-10` (:180) is undecidable where specRef lies
    within its own float32 error of the cut -- and matters only where the diffuse term does not swamp it."""
    n = len(wo)
    up = ~((wi[:, 2] <= 0) | (wo[:, 2] <= 0))                                           # :145-146: a NaN passes this test
    H = wi + wo
    ax, ay, kd, ks = P[1], P[2], P[3], P[4]
    model = int(P[0])
    cz = wi[:, 2] * wo[:, 2]
    if model == 0:                                                                     # :158-161
        factor1 = 1.0 / (4.0 * np.pi * ax * ay * np.sqrt(np.maximum(cz, 0)))
    elif model == 1:                                                                   # :162-165
        factor1 = 1.0 / (4.0 * np.pi * ax * ay * cz)
    elif model == 2:                                                                   # :166-169
        factor1 = _dot(H, H) / (np.pi * ax * ay * H[:, 2] ** 4)
    else:
        raise ValueError("unknown Ward model type %r" % model)
    x = _ward_exponent(P, H)
    spec_ref = factor1 * np.exp(x) * ks
    cs = 14 + 8 * np.abs(x)
    use = spec_ref > SPEC_CUT
    spec = np.where(use[:, None], _rgb(P, 10) * spec_ref[:, None], 0.0)
    diff = np.broadcast_to(_rgb(P, 7) * (kd / np.pi), (n, 3))                          # :184-185
    val = spec + diff
    cond = np.max([_mix_cond([(spec[:, c], cs), (diff[:, c], 4.0 * np.ones(n))]) for c in range(3)], axis=0)
    near_cut = np.abs(spec_ref - SPEC_CUT) < SPEC_CUT * (MARGIN + DIR_REACH * EPS32 * cs)
    amb = np.zeros(n, dtype=bool)
    for c in range(3):
        amb |= _relevant(near_cut & (P[10 + c] != 0), P[10 + c] * SPEC_CUT * np.ones(n), diff[:, c])
    return np.where(up[:, None], val, 0.0), np.where(up, cond, 1.0), up & amb


def ward_pdf_spec(P, wi, wo):
    """Ward::pdfSpec (ward.cpp:190-199) -> (value, cond): <H, wi> = (1 + <wi, wo>) / |wi + wo| cancels when wo -> -wi"""
    Hs = wi + wo
    H = _normalize(Hs)
    hw = _dot(H, wi)
    factor1 = 1.0 / (4.0 * np.pi * P[1] * P[2] * hw * H[:, 2] ** 3)
    x = _ward_exponent(P, H)
    c_dot = np.abs(H * wi).sum(axis=1) / np.where(hw != 0, np.abs(hw), 1e-300)
    return factor1 * np.exp(x), 18 + 8 * np.abs(x) + 4 * c_dot


def ward_pdf(P, wi, wo):
    """Ward::pdf (ward.cpp:201-220) with both lobes -> (value, cond, amb)"""
    n = len(wo)
    up = ~((wi[:, 2] <= 0) | (wo[:, 2] <= 0))                                           # :207-208
    ps, cs = ward_pdf_spec(P, wi, wo)
    pd = wo[:, 2] / np.pi                                                              # pdfLambertian (:248-250)
    ssw, dsw = P[5], P[6]
    val = ssw * ps + dsw * pd
    cond = _mix_cond([(ssw * ps, cs), (dsw * pd, 4.0 * np.ones(n))])
    # float32 exp() underflows into the denormals beyond 87: only where that term is all there is
    amb = _relevant((_ward_exponent(P, wi + wo) < -86.0) & (ssw != 0), ssw * ps, dsw * pd)
    return np.where(up, val, 0.0), np.where(up, cond, 1.0), up & amb


def ward_sample(P, wi, s):
    """Ward::sample(bRec, sample) (ward.cpp:259-285) with sampleSpecular (:222-246) and sampleLambertian (:252-257), then
    the base class's re-evaluation (src/librender/bsdf.cpp:37-48).  Undecidable in float32: `sample.y > 0.5` (:225) near one
    half, the poles of tan(2 pi sample.y) at one and three quarters (the float32 product 2 pi sample.y lies on the other side
    of the pole than the exact one), and the side test `cosTheta(wo) <= 0` (:242) of the SPECULAR lobe where wo.z is within
    reach of its own rounding.  Decidable, although they look like thresholds:
    * `sample.x <= specularSamplingWeight` (:270) compares two binary32 INPUTS, so both readings agree on every record; it is
      flagged only within MARGIN of a weight strictly between 0 and 1, as ref64 does for Phong, and never for a weight of
      exactly 0 or 1.
    * the diffuse lobe has no side test: squareToHemispherePSA (util.cpp:572-588) returns z > 0 always (z == 0 is replaced by
      the normalised (x, y, Epsilon)), so at sample.x = 1 - 2^-24, where the stretched sample is within 2^-24 / dsw of 1 and
      wo lies on the rim, the sample succeeds in either precision with sampledType EDiffuseReflection; only the direction's
      z, about sqrt(1 - u), is beyond comparison (dir_cond = 4 + 1 / z^2).
    * specularSamplingWeight = 0 and sample.x = 0: 0 <= 0 takes the specular lobe with 0 / 0 = NaN, every later test
      (`wo.z <= 0`, `specRef > 1e-10`, isZero) is false for a NaN, so the reference returns wo = NaN, pdf = NaN and
      f = the diffuse term: `alive` follows the same tests, NaNs included."""
    r = Sample(len(s))
    ax, ay, ssw, dsw = P[1], P[2], P[5], P[6]
    u = s.copy()
    spec = u[:, 0] <= ssw
    u[:, 0] = np.where(spec, u[:, 0] / ssw, (u[:, 0] - ssw) / dsw)
    # --- sampleSpecular ---
    phi = np.arctan(ay / ax * np.tan(2.0 * np.pi * u[:, 1]))
    phi = np.where(u[:, 1] > 0.5, phi + np.pi, phi)
    cph = np.cos(phi)
    sph = np.sqrt(np.maximum(0.0, 1.0 - cph * cph))
    L = -np.log(u[:, 0])
    th = np.arctan(np.sqrt(np.maximum(0.0, L / ((cph * cph) / (ax * ax) + (sph * sph) / (ay * ay)))))
    H = np.stack([np.sin(th) * np.cos(phi), np.sin(th) * np.sin(phi), np.cos(th)], axis=1)      # util.cpp:543-550
    ws = H * (2.0 * _dot(wi, H))[:, None] - wi
    amax, amin = max(ax, ay), min(ax, ay)
    # theta: -log(u) loses u's rounding absolutely (eps / sqrt(L) alpha in theta); the denominator subtracts in 1 - cos^2
    # ((amax / amin)^2 eps); phi: the argument of tan carries 2 pi eps, stretched by at most max(r, 1 / r), r = alphaY / alphaX
    dcs = 24 + 2 * amax / np.sqrt(np.maximum(L, 1e-300)) + (amax / amin) ** 2 + 16 * amax / amin
    # --- sampleLambertian ---
    wd, dcd = square_to_hemisphere_psa(u)
    r.wo = np.where(spec[:, None], ws, wd)
    r.stype = np.where(spec, GLOSSY_REFL, DIFFUSE_REFL)
    r.dir_cond = np.where(spec, dcs / np.where(ssw > 0, ssw, 1), dcd / np.where(dsw > 0, dsw, 1))
    fv, _, fa = ward_f(P, wi, r.wo)
    pv, _, pa = ward_pdf(P, wi, r.wo)
    # sample(bRec, s) returns f / pdf unless wo.z <= 0 (:242, specular lobe only); bsdf.cpp:38 asks whether that is zero
    qv = fv * (1.0 / pv)[:, None]
    r.alive = ~(wi[:, 2] <= 0) & ~(spec & (r.wo[:, 2] <= 0)) & ~(qv == 0).all(axis=1)
    poles = (np.abs(u[:, 1] - 0.25) < MARGIN) | (np.abs(u[:, 1] - 0.75) < MARGIN) | (np.abs(u[:, 1] - 0.5) < MARGIN)
    lobe = (np.abs(s[:, 0] - ssw) < MARGIN) & (0 < ssw < 1)
    r.amb = lobe | (spec & poles) | fa | pa
    r.side_test = spec                           # which records went through the side test of :242
    return r


class Table:
    """A BSDF table (types [n], params [n][16]) and f / pdf / sample of its entries"""

    # what a Table lends to a check that takes the ref64 module
    EPS32, DIR_REACH, MARGIN = EPS32, DIR_REACH, MARGIN
    point_light = staticmethod(ref64.point_light)

    def __init__(self, types=(), params=()):
        self.types = [int(t) for t in types]
        self.params = [np.asarray(p, dtype=np.float32) for p in params]

    # --- composite helpers -------------------------------------------------------------------------------------------
    def _children(self, P):
        n = int(P[0])
        w = np.asarray(P[1:1 + n], dtype=np.float64)
        idx = [int(P[1 + n + i]) for i in range(n)]
        return n, w, idx

    @staticmethod
    def _knots(w):
        """DiscretePDF::build (pdf.h:82-95): m_cdf[0..n] and the normalised m_pdf"""
        acc = np.concatenate([[0.0], np.cumsum(w)])
        total = acc[-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            cdf = acc / total
            p = w / total
        cdf[-1] = 1.0
        return cdf, p

    # --- f ------------------------------------------------------------------------------------------------------------
    def f(self, btype, P, wi, wo):
        base = btype & 0xFF
        if base not in (WARD, COMPOSITE):
            return ref64.f(btype, P, wi, wo)
        P = _f64(P); wi = _f64(wi).reshape(-1, 3); wo = _f64(wo).reshape(-1, 3)
        n = len(wo); wi = np.broadcast_to(wi, (n, 3)).copy()
        if btype & TWOSIDED:                                                            # twosided.cpp:80-88
            flip = wi[:, 2] < 0
            wi[flip, 2] *= -1; wo = wo.copy(); wo[flip, 2] *= -1
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if base == WARD:
                return ward_f(P, wi, wo)
            # Composite::f (composite.cpp:144-159): sum of f_i * w_i in table order
            k, w, idx = self._children(P)
            vals = [self.f(self.types[c], self.params[c], wi, wo) for c in idx]
            val = sum(v[0] * w[i] for i, v in enumerate(vals))
            cond = np.max([_mix_cond([(v[0][:, c] * w[i], v[1]) for i, v in enumerate(vals)]) for c in range(3)], axis=0) + 2 * k
            amb = np.zeros(n, dtype=bool)
            for i, v in enumerate(vals):
                rest = val - v[0] * w[i]
                amb |= _relevant(v[2] & (w[i] != 0), np.abs(v[0] * w[i]).max(axis=1), np.abs(rest).max(axis=1))
            return val, cond, amb

    # --- pdf ----------------------------------------------------------------------------------------------------------
    def pdf(self, btype, P, wi, wo):
        base = btype & 0xFF
        if base not in (WARD, COMPOSITE):
            return ref64.pdf(btype, P, wi, wo)
        P = _f64(P); wi = _f64(wi).reshape(-1, 3); wo = _f64(wo).reshape(-1, 3)
        n = len(wo); wi = np.broadcast_to(wi, (n, 3)).copy()
        if btype & TWOSIDED:                                                            # twosided.cpp:90-98
            flip = wi[:, 2] < 0
            wi[flip, 2] *= -1; wo = wo.copy(); wo[flip, 2] *= -1
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if base == WARD:
                return ward_pdf(P, wi, wo)
            # Composite::pdf (composite.cpp:178-193): sum of pdf_i * m_pdf[i]
            k, w, idx = self._children(P)
            _, p = self._knots(w)
            vals = [self.pdf(self.types[c], self.params[c], wi, wo) for c in idx]
            val = sum(v[0] * p[i] for i, v in enumerate(vals))
            cond = _mix_cond([(v[0] * p[i], v[1]) for i, v in enumerate(vals)]) + 2 * k
            amb = np.zeros(n, dtype=bool)
            for i, v in enumerate(vals):
                amb |= _relevant(v[2] & (p[i] != 0), v[0] * p[i], val - v[0] * p[i])
            return val, cond, amb

    # --- sample(bRec, pdf, s) -----------------------------------------------------------------------------------------
    def sample(self, btype, P, wi, s):
        base = btype & 0xFF
        if base not in (WARD, COMPOSITE):
            return ref64.sample(btype, P, wi, s)
        P = _f64(P); wi = _f64(wi).reshape(-1, 3); s = _f64(s).reshape(-1, 2)
        n = len(s); wi = np.broadcast_to(wi, (n, 3)).copy()
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            if btype & TWOSIDED:                                                        # twosided.cpp:115-127
                flip = wi[:, 2] < 0
                wi[flip, 2] *= -1
                r = self.sample(base, P, wi, s)
                r.wo[flip & r.alive, 2] *= -1
                return r
            if base == WARD:
                r = ward_sample(P, wi, s)
                reach = MARGIN + DIR_REACH * EPS32 * np.where(np.isfinite(r.dir_cond), r.dir_cond, 0)
                r.amb = r.amb | (r.side_test & (np.abs(r.wo[:, 2]) < reach))
                return r
            return self._sample_composite(P, wi, s)

    def _sample_composite(self, P, wi, s):
        """Composite::sample(bRec, pdf, sample) (composite.cpp:212-229): m_pdf.sampleReuse(sample.x) (pdf.h:102-107,
        :128-133) picks the child, the child's sample(bRec, sample) the direction -- a zero spectrum fails the sample --, then
        pdf() and f() of the whole composite at that direction.  The interval edges m_cdf[1..n-1] are float32 quotients: a
        sample within reach of one may pick either neighbour (m_cdf[0] = 0 and m_cdf[n] = 1 are exact, and decide nothing unless
        the first weight is zero)."""
        n = len(s)
        k, w, idx = self._children(P)
        cdf, p = self._knots(w)
        # std::lower_bound: the first knot that is not below the sample
        entry = np.clip(np.searchsorted(cdf, s[:, 0], side="left") - 1, 0, k - 1)
        lo, hi = cdf[entry], cdf[entry + 1]
        u = s.copy()
        u[:, 0] = (s[:, 0] - lo) / (hi - lo)
        r = Sample(n)
        amb = np.zeros(n, dtype=bool)
        for j in range(1, k):
            amb |= np.abs(s[:, 0] - cdf[j]) < MARGIN
        if w[0] == 0:
            amb |= s[:, 0] < MARGIN
        amb |= ~(hi - lo > 0)
        for i, c in enumerate(idx):
            sel = entry == i
            if not sel.any():
                continue
            ch = self.sample(self.types[c], self.params[c], wi[sel], u[sel])
            r.wo[sel] = ch.wo; r.stype[sel] = ch.stype; r.alive[sel] = ch.alive
            # the reused sample carries the rounding of the two knots, stretched by the interval's width
            r.dir_cond[sel] = ch.dir_cond * 2.0 / np.maximum(hi[sel] - lo[sel], 1e-300)
            amb[sel] |= ch.amb
        fv, _, fa = self.f(COMPOSITE, P, wi, r.wo)
        pv, _, pa = self.pdf(COMPOSITE, P, wi, r.wo)
        r.alive = r.alive & fv.any(axis=1) & (pv != 0)
        r.amb = amb | (r.alive & (fa | pa))
        return r

    # --- what path.cpp:100-125 adds at the first hit for a delta luminaire (ref64.direct_radiance with this table) -------
    def direct_radiance(self, btype, P, frame, wi_world, d, value):
        F = np.asarray(frame, dtype=np.float64)
        wi = wi_world @ F.T if F.ndim == 2 else np.einsum("nij,nj->ni", F, wi_world)
        wo = (-d) @ F.T if F.ndim == 2 else np.einsum("nij,nj->ni", F, -d)
        fv, _, _ = self.f(btype, P, wi, wo)
        return value * fv * np.abs(wo[:, 2])[:, None]


def table_of(sd):
    """the Table of a scene description's BSDF blocks"""
    return Table(sd.bsdf_type, sd.bsdf_params)
