"""integration/streamparse.h and the `vertexcolors` texture, on bytes: streams written by tests/mts_stream_writer_vcol.py with a
VertexColors instance in each texture slot of each class -> the slot mask next to the block, and a block equal bit for bit to
the one the same stream gives with constant (1, 1, 1) textures; what is refused (shared instances, roughglass' alpha, a
composite child, every other texture class as before)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_vcol as WV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [0, 1, 2, 3, 5, 6, 7, 8]            # Mirror keeps a plain Spectrum (mirror.cpp:51-55): no texture to replace


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_vcol") / "libstreamharness_vcol.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_vcol.cpp"), "-o", so])
    return C.CDLL(so)


def _parse(sp, data, prec=4, cap=16):
    types = np.zeros(cap, dtype=np.uint32); params = np.zeros((cap, 16), dtype=np.float32); slots = np.zeros(cap, dtype=np.uint32)
    n, own = C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    u32p = C.POINTER(C.c_uint32)
    rc = sp.sp_parse_bsdf_table_vcol(buf, C.c_size_t(len(data)), prec, types.ctypes.data_as(u32p), params.ctypes.data_as(C.POINTER(C.c_float)),
                                     slots.ctypes.data_as(u32p), cap, C.byref(n), C.byref(own), msg, C.c_size_t(512))
    return rc, msg.value.decode(errors="replace"), types[:n.value], params[:n.value], slots[:n.value], own.value


def _block(mts, btype, mask):
    """the block the scene-description mirror builds for type `btype` with VERTEX_COLORS in the slots of `mask` (mask 0: the
    constants 1 there), Phong / Ward after their configure()"""
    sd = mts.scenes.SceneDescription("b")
    V = mts.scenes.VERTEX_COLORS
    a, b = (V if mask & 1 else 1.0), (V if mask & 2 else 1.0)
    i = {0: lambda: sd.lambertian(a), 1: lambda: sd.dielectric(1.4, 1.1, refl=a, trans=b), 2: lambda: sd.roughmetal(0.2, 0.4, 2.5, refl=a),
         3: lambda: sd.microfacet(0.15, 0.4, 0.3, 1.6, 1.0, rd=a, rs=b), 5: lambda: sd.phong(17.0, rd=a, rs=b, kd=0.6, ks=0.7),
         6: lambda: sd.roughglass(0.2, 1.5, 1.0, "ggx", refl=a, trans=b), 7: lambda: sd.difftrans(a),
         8: lambda: sd.ward(0.2, 0.2, rd=a, rs=b, kd=0.8, ks=0.9, model="ward-duer")}[btype]()
    return sd.bsdf_params[i], sd.bsdf_color_slots[i]


@pytest.mark.parametrize("prec", [4, 8])
@pytest.mark.parametrize("btype", TYPES)
def test_vertex_colors_in_every_slot(sp, mts, prec, btype):
    n_slots = len(mts.abi.BSDF_COLOR_SLOTS[btype])
    P1, zero = _block(mts, btype, 0)
    assert zero == 0
    for two in (False, True):
        for tex_parent in (False, True):
            s = W.Stream(prec); WV.bsdf(s, "b", btype, P1, 0, twosided=two, tex_parent=tex_parent)
            rc, msg, t0, B0, m0, own = _parse(sp, s.bytes(), prec)
            assert rc == 0 and own == 0 and m0.tolist() == [0], msg
            for mask in range(1, 1 << n_slots):
                Pm, mirror_mask = _block(mts, btype, mask)
                assert mirror_mask == mask
                # Phong / Ward: the coloured block of the mirror IS the constant-1 block (getAverage() = 1), so the writer
                # can take its configure()d weights from either
                assert np.array_equal(Pm.view(np.uint32), P1.view(np.uint32))
                # constants that are NOT 1 in the coloured slots: the parser must not read them (nothing is in the stream)
                Pw = Pm.copy()
                for k, o in enumerate(mts.abi.BSDF_COLOR_SLOTS[btype]):
                    if mask >> k & 1: Pw[o:o + 3] = 0.123
                s = W.Stream(prec); WV.bsdf(s, "b", btype, Pw, mask, twosided=two, tex_parent=tex_parent)
                rc, msg, t, B, m, own = _parse(sp, s.bytes(), prec)
                assert rc == 0 and own == 0 and len(t) == 1, msg
                assert int(t[0]) == (btype | (0x100 if two else 0)) == int(t0[0])
                assert m.tolist() == [mask], (btype, mask, m)
                assert np.array_equal(B[0].view(np.uint32), B0[0].view(np.uint32)), (btype, mask, B[0], B0[0])
                # a caller that takes no masks is told, not handed a white BSDF
                msgb = C.create_string_buffer(512)
                data = s.bytes(); buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
                assert sp.sp_parse_bsdf_table_plain(buf, C.c_size_t(len(data)), prec, msgb, C.c_size_t(512)) == 1
                assert "does not take colour slots" in msgb.value.decode()


def test_refusals(sp, mts):
    P, _ = _block(mts, 5, 0)
    s = W.Stream(); WV.bsdf(s, "b", 5, P, 3, share=True)
    rc, msg, t, *_ = _parse(sp, s.bytes())
    assert rc == 1 and len(t) == 0 and "shared" in msg and "VertexColors" in msg, msg
    G, _ = _block(mts, 6, 0)
    s = W.Stream(); WV.bsdf(s, "b", 6, G, 0, alpha_colors=True)
    rc, msg, *_ = _parse(sp, s.bytes())
    assert rc == 1 and "alpha of RoughGlass is a VertexColors texture" in msg and "float texture" in msg, msg
    # every other texture class exactly as before
    for cls in ("BitmapTexture", "Checkerboard", "GridTexture"):
        s = W.Stream(); WV.bsdf(s, "b", 0, _block(mts, 0, 0)[0], 1, other_class=cls)
        rc, msg, *_ = _parse(sp, s.bytes())
        assert rc == 1 and "only constant" in msg and cls in msg, msg
    # a composite child with a coloured slot, named by its number; the same children without colours are fine
    L, _ = _block(mts, 0, 0)
    for mask, ok in ((0, True), (2, False)):
        s = W.Stream(); WV.composite(s, "c", [0.4, 0.6], [(("k", 0), 0, L, 0), (("k", 1), 5, P, mask)])
        rc, msg, t, B, m, own = _parse(sp, s.bytes())
        if ok:
            assert rc == 0 and own == 2 and m.tolist() == [0, 0, 0], msg
        else:
            assert rc == 1 and len(t) == 0 and len(m) == 0 and "child 1 (Phong) takes vertex colours" in msg, msg
    # truncated inside the VertexColors object
    s = W.Stream(); WV.bsdf(s, "b", 0, L, 1)
    good = s.bytes()
    for cut in (1, 3, 6, 14):
        rc, msg, *_ = _parse(sp, good[:-cut])
        assert rc == 1 and "end of the serialized stream" in msg, (cut, msg)


def test_masks_pass_the_library_check(mts):
    """what the parser reports is what mtsgpu_set_vertex_colors accepts: the table of include/mtsgpu.h on both sides"""
    for btype in TYPES:
        n_slots = len(mts.abi.BSDF_COLOR_SLOTS[btype])
        assert n_slots in (1, 2)
    assert mts.abi.BSDF_COLOR_SLOTS[4] == (0,) and mts.abi.BSDF_COLOR_SLOTS[9] == ()
