"""The sky luminaire's case list, shared by the CPU suite (tests/test_sky.py: host-side configure, the ambiguity cap) and
the device comparison (tests/test_gpu_sky.py): parameter sets, query directions with their edge classes, sample inputs.
Test infrastructure."""
import numpy as np

import closed_forms as cf
import ref64_sky

F = np.float32


def _rot(axis, deg):
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    t = np.radians(deg); c, s = np.cos(t), np.sin(t)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) * c + s * K + (1 - c) * np.outer(a, a)).astype(np.float32)


def parameter_sets(mts):
    """(name, block[32]) with the bounding sphere a flattener would have derived filled in by hand (centre, radius)"""
    specs = [
        ("defaults (sun below the horizon, 22:00)", dict()),
        ("sun at zenith, turbidity 2", dict(sun_direction=(0.0, 0.0, 1.0), turbidity=2.0)),
        ("sun at zenith, clip off", dict(sun_direction=(0.0, 0.0, 1.0), turbidity=3.0, clip_below_horizon=False)),
        ("sun low, turbidity 6", dict(sun_direction=(0.9, 0.3, 0.08), turbidity=6.0)),
        ("sun low, clip off, turbidity 10", dict(sun_direction=(-0.5, 0.8, 0.05), turbidity=10.0, clip_below_horizon=False)),
        ("sun below the horizon, clip off", dict(sun_direction=(0.4, -0.6, -0.3), turbidity=4.0, clip_below_horizon=False)),
        ("noon in summer, turbidity 3", dict(latitude=35.0, longitude=-100.0, standard_meridian=-105.0, julian_day=172.0,
                                             time_of_day=12.5, turbidity=3.0)),
        ("morning in winter, skyScale .25", dict(latitude=48.1, longitude=11.6, standard_meridian=15.0, julian_day=20.0,
                                               time_of_day=9.75, turbidity=2.5, sky_scale=0.25)),
        ("rotated toWorld", dict(sun_direction=(0.3, 0.2, 0.8), turbidity=4.0, to_world=_rot((0.3, 1.0, -0.2), 40.0))),
        ("rotated toWorld, clip off, skyScale 3", dict(sun_direction=(-0.2, 0.5, 0.4), turbidity=5.0, sky_scale=3.0,
                                                      clip_below_horizon=False, to_world=_rot((1.0, 0.2, 0.4), -115.0))),
        ("scaled a..e", dict(sun_direction=(0.1, -0.4, 0.6), turbidity=3.0, a=1.3, b=0.7, c=1.5, d=0.8, e=1.2)),
        ("scaled a..e, turbidity 8", dict(sun_direction=(0.6, 0.1, 0.3), turbidity=8.0, a=0.6, b=1.4, c=0.5, d=1.25, e=0.4, sky_scale=0.5)),
    ]
    out = []
    for name, kw in specs:
        sd = mts.scenes.SceneDescription("sky cases")
        l = sd.sky(**kw)
        P = sd.lum_params[l].copy()
        P[3:6] = [0.25, 1.0, -0.5]; P[6] = F(7.5)
        out.append((name, P))
    return out


def _world(P, local):
    """luminaire-space directions -> world (float32): the transpose of the block's world->luminaire rotation"""
    M = np.asarray(P[7:16], dtype=np.float64).reshape(3, 3)
    return (np.asarray(local, dtype=np.float64) @ M).astype(np.float32)         # M^T applied to columns


def directions(P, rng, n=4000):
    """-> (dirs [m][3] float32, classes {name: index array}): random directions, then the edges.  `horizon +- 1 ulp` are world
    directions whose luminaire-space z is the smallest binary32 step either side of 0 (as far as a rotation allows: the
    nudge is made in luminaire space and carried to world space)."""
    rnd = cf.square_to_sphere(np.ascontiguousarray(rng.random_sample((n, 2)), dtype=np.float32)) * F(1.0)
    rnd[: n // 4] *= rng.uniform(0.01, 50.0, (n // 4, 1)).astype(np.float32)            # Le(direction) normalises
    th_s, ph_s = float(P[16]), float(P[17])
    sun = np.array([np.sin(th_s) * np.cos(ph_s), np.sin(th_s) * np.sin(ph_s), np.cos(th_s)])
    k = 64
    az = rng.random_sample(k) * 2 * np.pi
    ring = np.stack([np.cos(az), np.sin(az), 0 * az], axis=1)
    tiny = float(np.nextafter(F(0), F(1)))
    off = np.array([0.0, 1e-6, 1e-4, 1e-3, 1e-2, 0.1])
    t1 = np.cross(sun, [0.3, -0.5, 0.8]); t1 /= np.linalg.norm(t1)

    def near(v):
        return np.stack([v + o * t1 for o in off])

    groups = [
        ("zenith", [[0, 0, 1.0], [1e-4, 0, 1.0], [0, -1e-3, 1.0], [1e-2, 1e-2, 1.0]]),
        ("horizon + 1 ulp", ring + [0, 0, tiny]),
        ("horizon - 1 ulp", ring - [0, 0, tiny]),
        ("horizon", ring),
        ("just above the horizon", np.concatenate([ring + [0, 0, h] for h in (2e-4, 9.99e-4, 1.001e-3, 3e-3, 2e-2)])),
        ("just below the horizon", np.concatenate([ring - [0, 0, h] for h in (2e-4, 1e-3, 2e-2)])),
        ("straight down", [[0, 0, -1.0], [1e-3, 0, -1.0], [0, 1e-2, -1.0]]),
        ("sun direction", near(sun)),
        ("antipode of the sun", near(-sun)),
    ]
    dirs, classes, at = [rnd], {"random": np.arange(n)}, n
    for name, g in groups:
        g = _world(P, np.asarray(g, dtype=np.float64).reshape(-1, 3))
        classes[name] = np.arange(at, at + len(g)); at += len(g)
        dirs.append(g)
    return np.concatenate(dirs).astype(np.float32), classes


def sample_points(rng, n):
    return (rng.uniform(-3.0, 3.0, (n, 3))).astype(np.float32)


def ambiguity(P, dirs):
    """records of Le the restatement cannot decide in binary32, every flagged record counted, black ones included"""
    val, cond, amb = ref64_sky.le(P, dirs)
    return amb, val
