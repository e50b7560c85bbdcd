"""The readers of integration/streamparse.h for Ward::serialize and Composite::serialize on bytes: streams written by
tests/mts_stream_writer_ward.py (an independent writer that follows the two serialize() methods) -> table entries that must
equal what the library's flattener keeps for the same scene description, bit for bit; both Float precisions, truncated
streams, and every composite the device cannot run."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_ward as WW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_table") / "libstreamharness_table.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_table.cpp"), "-o", so])
    return C.CDLL(so)


def _parse(sp, data, prec=4, cap=16):
    types = np.zeros(cap, dtype=np.uint32); params = np.zeros((cap, 16), dtype=np.float32)
    n, own = C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    rc = sp.sp_parse_bsdf_table(buf, C.c_size_t(len(data)), prec, types.ctypes.data_as(C.POINTER(C.c_uint32)),
                                params.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(n), C.byref(own), msg, C.c_size_t(512))
    return rc, msg.value.decode(errors="replace"), types[:n.value], params[:n.value], own.value


def _scene(mts):
    """a Ward of every model type, a twosided Ward, the xml's composite, a three-child composite with a twosided child and a
    twosided composite, all on spheres (two of the Wards are anisotropic)"""
    sd = mts.scenes.SceneDescription("streams")
    out = {}
    out["ward"] = sd.ward(0.1, 0.3, rd=(0.8, 0.4, 0.2), rs=(0.3, 0.9, 0.6), kd=0.9, ks=0.7, model="ward")
    out["duer"] = sd.ward(0.2, 0.2, model="ward-duer", specular_sampling_weight=0.25)
    out["balanced"] = sd.ward()
    out["two"] = sd.twosided(sd.ward(0.3, 0.1, rd=0.5, rs=0.5, kd=0.5, ks=0.5))
    phong = sd.phong(20.0, rd=1.0, rs=1.0, kd=0.5, ks=0.5)
    xml_ward = sd.ward(0.1, 0.3, rd=1.0, rs=1.0, kd=0.5, ks=0.5)
    out["xml"] = sd.composite([0.4, 0.6], [phong, xml_ward])
    lam, metal, tw = sd.lambertian(0.5, 0.6, 0.7), sd.roughmetal(0.1), sd.twosided(sd.ward(0.2, 0.2))
    out["three"] = sd.twosided(sd.composite([0.3, 0.0, 0.7], [lam, metal, tw]))
    for k, b in enumerate(out.values()):
        sd.add_sphere((2.5 * k, 0.0, 0.0), 1.0, bsdf=b)
    sd.point_light((0.0, 5.0, 0.0), 1.0)
    return sd, out


@pytest.mark.parametrize("prec", [4, 8])
@pytest.mark.parametrize("form", ["constants", "children", "shared"])
def test_ward_blocks_from_bytes(sp, mts, prec, form):
    sd, idx = _scene(mts)
    fa = mts.Scene(sd).arrays()
    for name in ("ward", "duer", "balanced", "two"):
        b = idx[name]
        t, P = int(fa["bsdf_type"][b]), np.array(fa["bsdf_params"][b], dtype=np.float32)
        if form == "shared":
            P = P.copy(); P[10:13] = P[7:10]             # one texture object in both slots: the second reference is a bare id
        s = W.Stream(prec)
        if t & 0x100:
            def body(s, P=P):
                W.configurable(s); s.string("m")
                WW.ward(s, "n", P, "m", tex_parent=(form == "children"), share_textures=(form == "shared"))
            s.ref("b", "TwoSidedBRDF", body)
        else:
            WW.ward(s, "b", P, "m", tex_parent=(form == "children"), share_textures=(form == "shared"))
        rc, msg, gt, gP, own = _parse(sp, s.bytes(), prec)
        assert rc == 0 and own == 0 and len(gt) == 1, msg
        assert int(gt[0]) == t
        assert np.array_equal(gP[0].view(np.uint32), P.view(np.uint32)), (name, gP[0], P)


@pytest.mark.parametrize("prec", [4, 8])
def test_composite_tables_from_bytes(sp, mts, prec):
    """children first, in their order, then the composite: its block holds their indices in the parsed table; entry by entry
    the parsed table equals the flattener's blocks of the same children"""
    sd, idx = _scene(mts)
    fa = mts.Scene(sd).arrays()
    T, PP = fa["bsdf_type"], fa["bsdf_params"]
    for name in ("xml", "three"):
        b = idx[name]
        n = int(PP[b][0]); weights = [float(w) for w in PP[b][1:1 + n]]; kids = [int(c) for c in PP[b][1 + n:1 + 2 * n]]
        s = W.Stream(prec)
        WW.composite(s, "c", weights, [(("kid", i), int(T[c]), PP[c]) for i, c in enumerate(kids)], name="mix", twosided=bool(int(T[b]) & 0x100))
        rc, msg, gt, gP, own = _parse(sp, s.bytes(), prec)
        assert rc == 0, msg
        assert len(gt) == n + 1 and own == n
        for i, c in enumerate(kids):
            assert int(gt[i]) == int(T[c])
            assert np.array_equal(gP[i].view(np.uint32), np.array(PP[c], dtype=np.float32).view(np.uint32)), (name, i)
        assert int(gt[n]) == int(T[b])
        want = np.zeros(16, dtype=np.float32); want[0] = n; want[1:1 + n] = PP[b][1:1 + n]; want[1 + n:1 + 2 * n] = np.arange(n)
        assert np.array_equal(gP[n].view(np.uint32), want.view(np.uint32))
        # the parsed table passes the library's own check of a BSDF table and flattens to itself
        sd2 = mts.scenes.SceneDescription("parsed")
        for t, P in zip(gt, gP):
            sd2.add_bsdf(int(t), P)
        sd2.add_sphere((0.0, 0.0, 0.0), 1.0, bsdf=own); sd2.point_light((0.0, 5.0, 0.0), 1.0)
        fb = mts.Scene(sd2).arrays()
        assert np.array_equal(fb["bsdf_params"].view(np.uint32), gP.view(np.uint32))


@pytest.mark.parametrize("prec", [4, 8])
def test_truncated_streams(sp, mts, prec):
    sd, idx = _scene(mts)
    s = W.Stream(prec); WW.ward(s, "b", sd.bsdf_params[idx["ward"]], "m")
    good = s.bytes()
    assert _parse(sp, good, prec)[0] == 0
    for cut in (1, prec, prec + 3, 6 * prec + 1, len(good) // 2, len(good) - 5):
        rc, msg, gt, _, own = _parse(sp, good[:-cut], prec)
        assert rc == 1 and own == -1 and len(gt) == 0 and "end of the serialized stream" in msg, (cut, msg)
        assert "Ward" in msg or cut > 6 * prec + 1              # the deepest cuts end inside the class name itself
    b = idx["xml"]; PP = sd.bsdf_params
    s = W.Stream(prec)
    WW.composite(s, "c", [0.4, 0.6], [(("k", 0), sd.bsdf_type[int(PP[b][3])], PP[int(PP[b][3])]), (("k", 1), 8, PP[int(PP[b][4])])])
    good = s.bytes()
    assert _parse(sp, good, prec)[0] == 0
    for cut in range(1, len(good) - 12, 7):
        rc, msg, gt, _, own = _parse(sp, good[:-cut], prec)
        assert rc == 1 and own == -1 and len(gt) == 0 and msg, (cut, msg)


def test_composites_the_device_cannot_run(sp, mts):
    lam = np.zeros(16, dtype=np.float32); lam[:3] = 0.5
    glass = np.float32([1.5, 1.0, 1, 1, 1, 1, 1, 1] + [0] * 8)
    def parse(weights, children):
        s = W.Stream(); WW.composite(s, "c", weights, children)
        return _parse(sp, s.bytes())
    rc, msg, *_ = parse([0.5, 0.5], [("a", 0, lam), ("b", 1, glass)])
    assert rc == 1 and "Dielectric" in msg and "delta BSDF" in msg
    rc, msg, *_ = parse([1.0], [("a", 4, lam)])
    assert rc == 1 and "Mirror" in msg and "delta BSDF" in msg
    rc, msg, *_ = parse([1.0], [("inner", 9, ([1.0], [("a", 0, lam)]))])
    assert rc == 1 and "nested composites" in msg
    rc, msg, *_ = parse([0.5, -0.5], [("a", 0, lam), ("b", 0, lam)])
    assert rc == 1 and "invalid BRDF weight" in msg
    rc, msg, *_ = parse([], [])
    assert rc == 1 and "between 1 and 7" in msg
    rc, msg, *_ = parse([0.1] * 8, [(("k", i), 0, lam) for i in range(8)])
    assert rc == 1 and "between 1 and 7" in msg
    rc, msg, *_ = parse([0.5, 0.5], [("a", 0, lam), ("a", 0, lam)])               # one instance twice: the second is a bare id
    assert rc == 1 and "shared instances" in msg
    rc, msg, *_ = parse([1.0], [(None, 0, lam)])
    assert rc == 1 and "missing" in msg
    # seven children are fine
    rc, msg, gt, gP, own = parse([0.1] * 7, [(("k", i), 0, lam) for i in range(7)])
    assert rc == 0 and own == 7 and len(gt) == 8
    # a class that is still not on the path, a bad Ward model type, and parseBSDF's refusal of a composite is by name
    s = W.Stream(); s.ref("b", "Mask", lambda s: (W.configurable(s), s.string("")))
    rc, msg, *_ = _parse(sp, s.bytes())
    assert rc == 1 and "Mask" in msg and "not on this path" in msg
    P = np.zeros(16, dtype=np.float32); P[0] = 3; P[1:7] = [0.1, 0.1, 1, 1, 0.5, 0.5]
    s = W.Stream(); WW.ward(s, "b", P)
    rc, msg, *_ = _parse(sp, s.bytes())
    assert rc == 1 and "unknown model type" in msg
