"""Case lists and checks that hold a float32 evaluator against tests/ref64.py: BSDF read-outs with the layout of
mtsgpu_bsdf_eval (the CPU suite hands in the oracle's, the GPU suite the device's) and single-quad renders lit by one
delta luminaire (oracle renders in the CPU suite, device renders in the GPU suite).  Test infrastructure."""
import numpy as np

import ref64
from chisquare_ref import bsdf_models, square_to_sphere

EPS = ref64.EPS32
# |got - ref| <= K_VALUE * 2^-23 * cond * |ref| + ATOL, cond = ref64's conditioning factor of each value.  When these
# checks were written the worst ratio over all models, f / pdf / sample weights, was 3.1 (microfacet pdf); K_VALUE
# leaves a factor of 5.  The failure messages print the worst ratio and its input.
K_VALUE = 16.0
K_DIR = float(ref64.DIR_REACH)                # sampled directions, componentwise: |got - ref| <= K_DIR * 2^-23 * dir_cond
ATOL = 1e-30                 # values this small are float32 denormals or flushed on the way
MAX_AMBIGUOUS = 0.05         # at most this share of the records may sit within float32 reach of a branch threshold


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _unit(v):
    v = _f32(v)
    return (v / np.sqrt((v * v).sum(axis=-1, keepdims=True))).astype(np.float32)


def parameter_sets(mts):
    """(name, bsdf_type, params): the chi-square models plus the edges of the parameter space"""
    sd = mts.scenes.SceneDescription("closed_forms")
    extra = [
        ("roughmetal alphaB .01", sd.roughmetal(0.01)),
        ("roughmetal alphaB 1", sd.roughmetal(1.0)),
        ("roughmetal k 0", sd.roughmetal(0.3, ior=1.5, k=0.0)),
        ("roughmetal coloured", sd.add_bsdf(2, [0.2, 0.2, 1.1, 0.9, 3.0, 2.4, 1.6, 0.9, 0.6, 0.3])),
        ("microfacet alphaB .01", sd.microfacet(0.01, 0.5, 0.5, 1.5, 1.0, 0.8, 1.0)),
        ("microfacet alphaB 1", sd.microfacet(1.0, 0.5, 0.5, 1.5, 1.0, 0.8, 1.0)),
        ("microfacet intIOR < extIOR", sd.microfacet(0.2, 0.3, 0.7, 1.0, 1.5, 0.8, 1.0)),
        ("phong exponent 1", sd.phong(1.0, rd=0.6, rs=0.4, kd=0.5, ks=0.5)),
        ("phong exponent 1000", sd.phong(1000.0, rd=0.6, rs=0.4, kd=0.5, ks=0.5)),
        ("phong exponent 300 specular only", sd.phong(300.0, rd=0.0, rs=1.0, kd=0.0, ks=1.0)),
        ("dielectric", sd.dielectric(1.5, 1.0)),
        ("dielectric intIOR < extIOR", sd.dielectric(1.0, 1.33)),
        ("mirror", sd.mirror(0.8)),
        ("roughglass beckmann .01", sd.roughglass(0.01, 1.5, 1.0, "beckmann")),
        ("roughglass ggx 1 intIOR < extIOR", sd.roughglass(1.0, 1.0, 1.5, "ggx")),
        ("twosided lambertian", sd.twosided(sd.lambertian(0.5))),
        ("twosided phong exponent 20", sd.twosided(sd.phong(20.0, rd=1.0, rs=1.0, kd=0.5, ks=0.5))),
    ]
    return ([(name, btype, params) for name, btype, params, _ in bsdf_models(mts)]
            + [(name, sd.bsdf_type[i], sd.bsdf_params[i]) for name, i in extra])


def _grazing(z, phi):
    return _unit(np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z + 0 * phi], axis=-1))


def direction_pairs(params, btype, rng, n=20000):
    """about n random pairs on the sphere followed by the edge list; returns wi, wo [m][3] float32"""
    wi = square_to_sphere(_f32(rng.random_sample((n, 2))))
    wo = square_to_sphere(_f32(rng.random_sample((n, 2))))
    k = 400
    up = square_to_hemisphere(rng, k)
    phis = rng.random_sample(k) * 2 * np.pi
    edges_i, edges_o = [], []
    def add(a, b):
        a, b = np.broadcast_arrays(_f32(a).reshape(-1, 3), _f32(b).reshape(-1, 3))
        edges_i.append(a); edges_o.append(b)
    add([0, 0, 1], up)                                          # normal incidence: tan(theta) = 0, G1 = 1
    add(up, [0, 0, 1])
    add([0, 0, 1], [0, 0, 1])
    for z in (1e-3, 1e-6):                                      # grazing incidence and exitance
        add(_grazing(z, phis), up)
        add(up, _grazing(z, phis))
        g = _grazing(z, phis)
        add(g, g * np.float32([-1, -1, 1]))                     # grazing mirror pair
    add(up, up * np.float32([-1, -1, 1]))                       # wo at the mirror direction of wi
    add(up, up)                                                 # wo = wi
    add(-up, up); add(up, -up); add(-up, -up)                  # below the surface: one side, the other, both
    add(up * np.float32([1, 1, -1]), up[::-1] * np.float32([1, 1, -1]))
    add(up, -up[::-1]); add(-up, up[::-1])                      # twosided with mixed signs
    add([0, 0, -1], up); add([0, 0, -1], -up)
    add(up, -up * np.float32([-1, -1, 1]))                      # wo = -wi: straight through
    add(-up, up * np.float32([-1, -1, 1]))
    # inside the dielectric, just below / at / beyond the critical angle (and the same from outside)
    for inte, ext in ((params[0], params[1]), (params[2], params[3])):
        if not (0.5 < inte < 3 and 0.5 < ext < 3) or inte == ext:
            continue
        sc = min(inte, ext) / max(inte, ext)
        for st in (sc * (1 - 1e-3), sc * (1 - 1e-6), sc, sc * (1 + 1e-6), sc * (1 + 1e-3), 0.999):
            if st >= 1:
                continue
            z = np.sqrt(1 - st * st)
            g = _grazing(z, phis[:50])
            add(g * np.float32([1, 1, -1]), up[:50]); add(g * np.float32([1, 1, -1]), -up[:50])
            add(g, up[:50]); add(g, -up[:50])
    return np.concatenate([wi] + edges_i), np.concatenate([wo] + edges_o)


def square_to_hemisphere(rng, k):
    v = square_to_sphere(_f32(rng.random_sample((k, 2))))
    v[:, 2] = np.abs(v[:, 2])
    return _unit(v)


def sample_inputs(rng, n):
    """random samples plus every coordinate at 0 and at 1 - 2^-24 (the largest float32 below 1)"""
    s = _f32(rng.random_sample((n, 2)))
    top = np.float32(1 - 2.0 ** -24)
    q = n // 5
    s[0:q, 0] = 0; s[q:2 * q, 0] = top; s[2 * q:3 * q, 1] = 0; s[3 * q:4 * q, 1] = top
    s[4 * q:4 * q + 4] = [[0, 0], [0, top], [top, 0], [top, top]]
    return s


def _check_values(report, what, got, ref, cond, sel):
    """|got - ref| <= K_VALUE eps cond |ref| + ATOL on the selected records; records the worst ratio.  A NaN or an
    infinity where the reference is finite has ratio inf."""
    got = np.asarray(got, dtype=np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, dtype=np.float64).reshape(len(ref), -1)
    cond = np.asarray(cond, dtype=np.float64).reshape(-1, 1)
    err = np.abs(got - ref) - ATOL
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        scale = EPS * cond * np.abs(ref)
        ratio = np.where(err > 0, err / np.where(scale > 0, scale, 1e-300), 0.0)
    ratio = np.where(~np.isfinite(got) & np.isfinite(ref), np.inf, ratio)
    ratio = np.where(sel[:, None], ratio, 0.0)
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    report.setdefault(what, [0.0, None])
    if ratio[worst] > report[what][0] or report[what][1] is None:
        report[what] = [float(ratio[worst]), int(worst[0])]
    return ratio.max(axis=1)


def _non_finite(failures, what, got, ref):
    """a NaN or infinity in a float32 result where the reference is finite (and within float32 range) is an error on
    every record, including those whose branch float32 cannot decide: no branch of these formulas yields one"""
    got = np.asarray(got).reshape(len(got), -1); ref = np.asarray(ref, dtype=np.float64).reshape(len(got), -1)
    with np.errstate(invalid="ignore"):
        bad = (~np.isfinite(got)).any(axis=1) & (np.isfinite(ref) & (np.abs(ref) < 1e38)).all(axis=1)
    if bad.any():
        failures.append("%s: %d non-finite results where the reference is finite, e.g. record %d: got %s ref %s"
                        % (what, bad.sum(), np.argmax(bad), got[np.argmax(bad)].tolist(), ref[np.argmax(bad)].tolist()))


def check_model(evaluate, name, btype, params, rng, n=20000, n_samples=20000):
    """compares f (op 0), pdf (op 1) and sample (op 2) of `evaluate` with ref64; returns (failures, report)"""
    params = _f32(params)
    failures, report = [], {}
    wi, wo = direction_pairs(params, btype, rng, n)
    amb_total, total = 0, 0
    # --- f and pdf ---
    for op, refn in ((0, ref64.f), (1, ref64.pdf)):
        got = evaluate(btype, params, op, wi, wo)
        val, cond, amb = refn(btype, params, wi, wo)
        val = np.asarray(val, dtype=np.float64).reshape(len(wi), -1)
        g = got[:, 0:3] if op == 0 else got[:, 0:1]
        _non_finite(failures, "%s op %d" % (name, op), g, val)
        amb_total += (amb & (np.abs(val) > 1e-20).any(axis=1)).sum(); total += len(amb)
        zero = (val == 0).all(axis=1) & ~amb
        bad = zero & (g != 0).any(axis=1)
        if bad.any():
            i = np.nonzero(bad)[0][0]
            failures.append("%s op %d: nonzero where the reference is exactly 0 (%d records), e.g. wi %s wo %s got %s"
                            % (name, op, bad.sum(), wi[i].tolist(), wo[i].tolist(), g[i].tolist()))
        sel = ~zero & ~amb & np.isfinite(val).all(axis=1)
        r = _check_values(report, ("f", "pdf")[op], g, val, cond, sel)
        if (r > K_VALUE).any():
            i = int(np.argmax(r))
            failures.append("%s op %d: worst ratio %.3g > %g at wi %s wo %s: got %s ref %s cond %.3g"
                            % (name, op, r[i], K_VALUE, wi[i].tolist(), wo[i].tolist(), g[i].tolist(), val[i].tolist(), cond[i]))
    # --- sample(bRec, pdf, s) ---
    swi = np.concatenate([wi[:n_samples], wi[n:]])
    s = sample_inputs(rng, len(swi))
    got = evaluate(btype, params, 2, swi, s)
    r = ref64.sample(btype, params, swi, s)
    gwo, gpdf, gf = got[:, 0:3], got[:, 3], got[:, 4:7]
    gtype = got[:, 7].copy().view(np.uint32)
    _non_finite(failures, "%s sample" % name, got[:, 0:7], np.concatenate([r.wo, r.pdf[:, None], r.f], axis=1))
    ok = ~r.amb
    galive = (gpdf != 0) & (gf != 0).any(axis=1)
    bad = ok & (galive != r.alive)
    if bad.any():
        i = np.nonzero(bad)[0][0]
        failures.append("%s sample: success differs from the reference on %d records, e.g. wi %s s %s: got %s pdf %g f %s, ref alive %s wo %s"
                        % (name, bad.sum(), swi[i].tolist(), s[i].tolist(), gwo[i].tolist(), gpdf[i], gf[i].tolist(), r.alive[i], r.wo[i].tolist()))
    dead = ~galive
    if ((gpdf[dead] != 0) | (gf[dead] != 0).any(axis=1)).any():
        failures.append("%s sample: a failed sample must report f = 0 and pdf = 0" % name)
    live = ok & r.alive & galive
    bad = live & (gtype != r.stype)
    if bad.any():
        i = np.nonzero(bad)[0][0]
        failures.append("%s sample: sampledType %#x != %#x at wi %s s %s" % (name, gtype[i], r.stype[i], swi[i].tolist(), s[i].tolist()))
    dsel = live & np.isfinite(r.dir_cond)
    with np.errstate(divide="ignore", invalid="ignore"):
        derr = np.abs(gwo - r.wo).max(axis=1) / (EPS * np.where(dsel, r.dir_cond, 1))
    derr = np.where(dsel & ~np.isfinite(gwo).all(axis=1), np.inf, derr)
    derr = np.where(dsel, derr, 0.0)
    report["direction"] = max(report.get("direction", [0.0, None]), [float(derr.max()), int(np.argmax(derr))])
    if (derr > K_DIR).any():
        i = int(np.argmax(derr))
        failures.append("%s sample: direction off by %.3g x eps x cond at wi %s s %s: got %s ref %s"
                        % (name, derr[i], swi[i].tolist(), s[i].tolist(), gwo[i].tolist(), r.wo[i].tolist()))
    if r.delta:
        # delta lobes: the weight is the sample's own, comparable where both took the same branch
        fv, fc, pv, pc = r.f, r.cond, r.pdf, r.cond
        sel = live
    else:
        # a re-evaluating sample(): f() and pdf() at the evaluator's own direction, wherever the evaluator succeeded
        fv, fc, fa = ref64.f(btype, params, swi, gwo)
        pv, pc, pa = ref64.pdf(btype, params, swi, gwo)
        sel = galive & ~(fa | pa)
        bad = sel & (((np.asarray(fv) == 0).all(axis=1)) | (np.asarray(pv) == 0))
        if bad.any():
            i = np.nonzero(bad)[0][0]
            failures.append("%s sample: a weight where the reference's f or pdf at the sampled wo is exactly 0, wi %s wo %s: f %s pdf %g"
                            % (name, swi[i].tolist(), gwo[i].tolist(), gf[i].tolist(), gpdf[i]))
    rf = _check_values(report, "sample f", gf, fv, fc, sel & (np.asarray(fv) != 0).any(axis=1))
    rp = _check_values(report, "sample pdf", gpdf, pv, pc, sel & (np.asarray(pv) != 0))
    for what, rr, gv, rv in (("f", rf, gf, fv), ("pdf", rp, gpdf, pv)):
        if (rr > K_VALUE).any():
            i = int(np.argmax(rr))
            failures.append("%s sample %s: worst ratio %.3g > %g at wi %s s %s wo %s: got %s ref %s"
                            % (name, what, rr[i], K_VALUE, swi[i].tolist(), s[i].tolist(), gwo[i].tolist(),
                               np.atleast_1d(gv[i]).tolist(), np.atleast_1d(rv[i]).tolist()))
    report["undecidable"] = "%d of %d f/pdf records, %d of %d samples" % (amb_total, total, (~ok).sum(), len(ok))
    if amb_total > MAX_AMBIGUOUS * total:
        failures.append("%s: %d of %d records undecidable in float32 -- the case list tests too little" % (name, amb_total, total))
    return failures, report


def assert_index_matched_roughglass(evaluate, distr):
    """roughglass with intIOR == extIOR: what the reference yields.
    f and pdf at wo = -wi: roughglass.cpp:375-376 (f) and :454-455 (pdf) build the transmission half-vector as
    normalize(wi * etaI + wo * etaT), here the zero vector; normalize() divides by its length (vector.h:403-405), so H is
    NaN, evalD(NaN) passes both of its zero tests (:210, :248) and f and pdf are NaN.  The reference gives NaN.
    A transmission sample (s.x = .95 is above the clamped Fresnel weight, :517-526) refracts through m with eta = 1
    (:182-196): wo = m (c - sqrt(1 + (c^2 - 1))) - wi.  sample(bRec, s) has a finite nonzero weight, and since
    roughglass.cpp:619 takes its pdf by value it overrides nothing: the base class (src/librender/bsdf.cpp:37-48)
    re-evaluates pdf() and f() at that wo.  Where binary32 rounding makes sqrt(1 + (c^2 - 1)) equal to c, wo is -wi
    bit for bit and f and pdf are NaN as above; otherwise wi + wo is a rounding residual that decides H: f and pdf are
    then zero exactly where the restatement's are at the evaluator's own wo (their size divides by the square of
    etaI <wi,H> + etaT <wo,H> = |wi + wo|, a pure rounding residual, and is not compared)."""
    P = _f32([distr, 0.3, 1, 1, 1, 1, 1, 1, 1, 1])
    rng = np.random.RandomState(11)
    wi = square_to_sphere(_f32(rng.random_sample((400, 2))))
    wi = np.concatenate([_unit([[0.3, -0.2, 0.9], [0.0, 0.0, 1.0], [0.6, 0.1, -0.5]]), wi])
    f = evaluate(6, P, 0, wi, -wi)[:, 0:3]
    p = evaluate(6, P, 1, wi, -wi)[:, 0]
    assert np.isnan(f).all() and np.isnan(p).all()
    assert np.isnan(ref64.f(6, P, wi, -wi)[0]).all() and np.isnan(ref64.pdf(6, P, wi, -wi)[0]).all()
    s = evaluate(6, P, 2, wi, np.tile(_f32([0.95, 0.3]), (len(wi), 1)))
    gwo, gpdf, gf = s[:, 0:3], s[:, 3], s[:, 4:7]
    exact = (gwo == -wi).all(axis=1)
    assert exact[1] and exact.sum() > 50                 # normal incidence, and many more
    assert np.isnan(gpdf[exact]).all() and np.isnan(gf[exact]).all()
    rest = ~exact
    fv, _, _ = ref64.f(6, P, wi[rest], gwo[rest])
    pv, _, _ = ref64.pdf(6, P, wi[rest], gwo[rest])
    alive = (pv != 0) & (fv != 0).any(axis=1)
    got_alive = (gpdf[rest] != 0) & (gf[rest] != 0).any(axis=1)
    assert np.array_equal(alive, got_alive)


# ---------------------------------------------------------------------------------------------------------------------
# Render-level closed forms: one floor quad (y = 0, normal +y), one delta luminaire, an orthographic camera, maxDepth 2,
# the box filter.  A camera sample's radiance is a function of its hit point alone (the continuation ray escapes and the
# luminaire has pdf 1), so every developed pixel lies between the extremes of ref64's closed form over its footprint.
# ---------------------------------------------------------------------------------------------------------------------
W = H = 24
SPP = 8
SUB = 17                 # closed form on SUB x SUB points of every footprint, edges and corners included
REL_TOL = 1e-4
# The closed form is known on the SUB x SUB grid only; between grid points it can reach past the grid's extremes.  For a
# smooth function the overshoot is at most h^2 |f''| / 8 with h = 1 / (SUB - 1) of the footprint, about 1/2000 of its
# variation (hi - lo) over the footprint for a quadratic peak: GRID_SLACK allows that with a margin, and keeps the
# interval of a pixel far narrower than the changes the render cases are there to see (a spot ramp linear in cos(theta)
# instead of the angle moves a ramp pixel by more than its whole interval).
GRID_SLACK = 0.005


def render_cases(mts):
    """(name, scene description, (btype, params), light closed form p -> (d, value), integrator)"""
    cases = []
    def scene(name, bsdf_fn, cam_origin, cam_target, scale=0.4):
        sd = mts.scenes.SceneDescription(name)
        b = bsdf_fn(sd)
        pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
        sd.add_mesh(pos, tri, bsdf=b, face_normals=True)
        up = (0.0, 0.0, -1.0) if abs(cam_origin[0] - cam_target[0]) + abs(cam_origin[2] - cam_target[2]) < 1e-6 else (0.0, 1.0, 0.0)
        sd.camera = dict(origin=cam_origin, target=cam_target, up=up, ortho_scale=(scale, scale))
        return sd, b
    def point(sd, pos, I):
        sd.point_light(pos, I)
        return lambda p: ref64.point_light([I] * 3, pos, p)
    oblique = ((1.2, 2.0, 0.9), (0.05, 0.0, -0.1))
    floors = [
        ("point light, lambertian floor", lambda sd: sd.add_bsdf(0, [0.5, 0.7, 0.2])),
        ("point light, phong 20 floor", lambda sd: sd.phong(20.0, rd=0.5, rs=0.5, kd=0.5, ks=0.5)),
        ("point light, microfacet .1 floor", lambda sd: sd.microfacet(0.1, 0.5, 0.5, 1.5, 1.0, 0.8, 1.0)),
        ("point light, roughmetal .1 floor", lambda sd: sd.roughmetal(0.1)),
        ("point light, roughglass reflection", lambda sd: sd.roughglass(0.3, 1.5, 1.0, "beckmann")),
    ]
    for name, fn in floors:
        sd, b = scene(name, fn, *oblique)
        L = point(sd, (-0.6, 1.5, -0.4), 6.0)
        cases.append((name, sd, b, L, "path"))
    # twosided phong seen from below, lit from below
    sd, b = scene("twosided phong from below", lambda sd: sd.twosided(sd.phong(20.0, rd=0.5, rs=0.5, kd=0.5, ks=0.5)),
                  (1.0, -2.0, 0.7), (0.0, 0.0, 0.0))
    cases.append(("twosided phong from below", sd, b, point(sd, (-0.5, -1.2, -0.3), 4.0), "path"))
    # spot light, beam 10 deg, cutoff 20 deg: flat core, ramp linear in the angle, zero outside (camera straight down)
    # the frame spans the edge of the core, the ramp and the dark beyond, in pixels narrow enough (a 15th of the ramp)
    # that a ramp linear in cos(theta) instead (up to .08 I away) falls outside the pixels' intervals
    sd, b = scene("spot light", lambda sd: sd.lambertian(0.5), (0.6, 3.0, -0.05), (0.6, 0.0, -0.05), scale=0.3)
    sd.spot_light((0.1, 2.0, -0.05), (0.1, 0.0, -0.05), 5.0, cutoff_deg=20.0, beam_deg=10.0)
    P = sd.lum_params[-1]
    spot = (lambda P: lambda p: ref64.spot_light([5.0] * 3, _f32(P[3:6]), _f32(P[10:19]), float(np.float32(P[8])),
                                                 float(np.float32(P[19])), p))(P.copy())
    cases.append(("spot light", sd, b, spot, "path"))
    # directional light at 30 degrees from the normal, glossy floor
    sd, b = scene("directional light", lambda sd: sd.phong(20.0, rd=0.5, rs=0.5, kd=0.5, ks=0.5), *oblique)
    d = _unit([np.sin(np.pi / 6), -np.cos(np.pi / 6), 0.0])
    sd.directional_light(d, 2.0)
    dd = sd.lum_params[-1][3:6].copy()
    cases.append(("directional light", sd, b, lambda p, dd=dd: ref64.directional_light([2.0] * 3, dd, p), "path"))
    # collimated beam of radius .3 hitting the floor obliquely
    sd, b = scene("collimated beam", lambda sd: sd.microfacet(0.2, 0.5, 0.5, 1.5, 1.0, 0.8, 1.0), (0.0, 3.0, 0.0), (0.0, 0.0, 0.0), scale=0.8)
    sd.collimated_beam((-1.5, 2.0, 0.2), (0.0, 0.0, 0.0), 3.0, radius=0.3)
    P = sd.lum_params[-1].copy()
    cases.append(("collimated beam", sd, b, lambda p, P=P: ref64.collimated_light([3.0] * 3, float(P[3]), P[4:16], P[16:28], p), "path"))
    # the same point-lit phong floor through the direct integrator
    sd, b = scene("direct integrator", lambda sd: sd.phong(20.0, rd=0.5, rs=0.5, kd=0.5, ks=0.5), *oblique)
    cases.append(("direct integrator", sd, b, point(sd, (-0.6, 1.5, -0.4), 6.0), "direct"))
    return cases


def footprints(cam):
    """world points [H][W][SUB*SUB][3] where the orthographic camera's rays through every pixel's SUB x SUB sub-grid hit
    the plane y = 0, and the (world) ray direction"""
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    u = np.linspace(0.0, 1.0, SUB)
    x = (np.arange(cam.width)[None, :, None, None] + u[None, None, :, None] + 0 * u[None, None, None, :])
    y = (np.arange(cam.height)[:, None, None, None] + 0 * u[None, None, :, None] + u[None, None, None, :])
    x, y = np.broadcast_arrays(x, y)
    ras = np.stack([x, y, 0 * x, 1 + 0 * x], axis=-1).reshape(-1, 4)
    pc = ras @ r2c.T; pc = pc[:, :3] / pc[:, 3:4]
    o = np.concatenate([pc, np.ones((len(pc), 1))], axis=1) @ c2w.T
    o = o[:, :3] / o[:, 3:4]
    d = c2w[:3, :3] @ np.array([0.0, 0.0, 1.0]); d /= np.linalg.norm(d)
    t = -o[:, 1] / d[1]
    p = o + t[:, None] * d
    return p.reshape(cam.height, cam.width, SUB * SUB, 3), d


def check_render(img, cam, btype, params, light):
    """every pixel within [min - tol, max + tol] of the closed form over its footprint (a NaN is outside); exactly 0
    where the whole footprint (widened by a sub-pixel) is unlit.  Returns (failures, worst excess relative to max,
    number of pixels checked for 0, number of pixels of the image with light)"""
    p, d = footprints(cam)
    flat = p.reshape(-1, 3)
    ld, val = light(flat)
    frame = np.array([[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0]])          # (s, t, n = +y): any frame will do, the BSDFs are isotropic
    wi = np.broadcast_to(-d, flat.shape)
    L = ref64.direct_radiance(btype, params, frame, wi, ld, val).reshape(p.shape[0], p.shape[1], -1, 3)
    lo, hi = L.min(axis=2), L.max(axis=2)
    tol = REL_TOL * np.maximum(hi, 1e-30) + GRID_SLACK * (hi - lo)
    failures = []
    if not np.isfinite(img).all():
        failures.append("%d non-finite values in the image" % (~np.isfinite(img)).sum())
    under = (lo - tol) - img
    over = img - (hi + tol)
    worst = float(np.max(np.maximum(under, over)) / max(hi.max(), 1e-30)) if np.isfinite(img).all() else np.inf
    bad = ~((img >= lo - tol) & (img <= hi + tol))
    if bad.any():
        y, x, c = np.argwhere(bad)[0]
        failures.append("pixel (%d, %d) channel %d: %.7g outside [%.7g, %.7g] (%d values outside)"
                        % (x, y, c, img[y, x, c], lo[y, x, c], hi[y, x, c], bad.sum()))
    # unlit: the footprint and its neighbours' all zero
    z = hi.max(axis=2) == 0
    zz = z.copy()
    zz[1:] &= z[:-1]; zz[:-1] &= z[1:]; zz[:, 1:] &= z[:, :-1]; zz[:, :-1] &= z[:, 1:]
    if (img[zz] != 0).any():
        failures.append("%d pixels in the unlit region are not exactly 0" % (img[zz] != 0).any(axis=1).sum())
    return failures, worst, int(zz.sum()), int((img > 0).any(axis=2).sum())
