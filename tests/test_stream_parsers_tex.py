"""integration/streamparse.h and the `checkerboard` / `gridtexture` textures, on bytes: streams written by
tests/mts_stream_writer_tex.py with a texture in each slot of each class -> the descriptor in the texture list, its index in
the slot table next to the block, and a block equal bit for bit to the scene-description mirror's (getAverage() in the slot);
what is refused (a shared instance, roughglass' alpha, a composite child, a caller that takes no textures)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_tex as WT
import mts_stream_writer_vcol as WV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [0, 1, 2, 3, 5, 6, 7, 8]            # Mirror keeps a plain Spectrum (mirror.cpp:51-55): no texture to replace


def _build(tmp, name, source):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp / name)
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", source), "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("harness_tex"), "libstreamharness_tex.so", "harness_tex.cpp")


def _parse(sp, mts, data, prec=4, cap=16):
    types = np.zeros(cap, dtype=np.uint32); params = np.zeros((cap, 16), dtype=np.float32); slots = np.zeros(cap, dtype=np.uint32)
    slot_tex = np.zeros((cap, 2), dtype=np.int32)
    tex = (mts.abi.UvTexture * cap)()
    n, nt, own = C.c_uint32(0), C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    u32p = C.POINTER(C.c_uint32)
    rc = sp.sp_parse_bsdf_table_tex(buf, C.c_size_t(len(data)), prec, types.ctypes.data_as(u32p), params.ctypes.data_as(C.POINTER(C.c_float)),
                                    slots.ctypes.data_as(u32p), slot_tex.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n), tex, cap, C.byref(nt),
                                    C.byref(own), msg, C.c_size_t(512))
    return rc, msg.value.decode(errors="replace"), types[:n.value], params[:n.value], slots[:n.value], slot_tex[:n.value], list(tex[:nt.value]), own.value


def _textures(mts):
    S = mts.scenes
    return (S.Checkerboard(bright=(0.8, 0.6, 0.4), dark=(0.2, 0.1, 0.3), uoffset=0.3, voffset=-0.3, uscale=3.7, vscale=-3.7),
            S.GridTexture(bright=(0.5, 0.25, 0.75), dark=(0.1, 0.05, 0.02), uoffset=-0.3, uscale=-3.7, vscale=2.0, line_width=0.07))


def _block(mts, btype, a, b):
    """the block and slot row the scene-description mirror builds for type `btype` with a, b in its texture slots"""
    sd = mts.scenes.SceneDescription("b")
    i = {0: lambda: sd.lambertian(a), 1: lambda: sd.dielectric(1.4, 1.1, refl=a, trans=b), 2: lambda: sd.roughmetal(0.2, 0.4, 2.5, refl=a),
         3: lambda: sd.microfacet(0.15, 0.4, 0.3, 1.6, 1.0, rd=a, rs=b), 5: lambda: sd.phong(17.0, rd=a, rs=b, kd=0.3, ks=0.2),
         6: lambda: sd.roughglass(0.2, 1.5, 1.0, "ggx", refl=a, trans=b), 7: lambda: sd.difftrans(a),
         8: lambda: sd.ward(0.2, 0.2, rd=a, rs=b, kd=0.3, ks=0.2, model="ward-duer")}[btype]()
    return sd.bsdf_params[i], sd.bsdf_slot_texture[i], sd.bsdf_color_slots[i]


def _same(d, t):
    return (d.kind == t.kind and [d.uoffset, d.voffset, d.uscale, d.vscale] == [t.uoffset, t.voffset, t.uscale, t.vscale]
            and list(d.bright) == list(t.bright) and list(d.dark) == list(t.dark) and (t.kind == 0 or d.line_width == t.line_width))


@pytest.mark.parametrize("prec", [4, 8])
@pytest.mark.parametrize("btype", TYPES)
def test_uv_textures_in_every_slot(sp, mts, prec, btype):
    S = mts.scenes
    check, grid = _textures(mts)
    n_slots = len(mts.abi.BSDF_COLOR_SLOTS[btype])
    choices = [None, check, grid, S.VERTEX_COLORS]
    for two in (False, True):
        for tex_parent in (False, True):
            for pick in range(len(choices) ** n_slots):
                arg = [choices[(pick // len(choices) ** k) % len(choices)] if k < n_slots else None for k in range(2)]
                slot_tex = [a if isinstance(a, S._UvTexture) else None for a in arg]
                mask = sum(1 << k for k, a in enumerate(arg) if a is S.VERTEX_COLORS)
                P, row, mirror_mask = _block(mts, btype, *[0.5 if a is None else a for a in arg])
                assert mirror_mask == mask
                # constants that are NOT the average in the textured slots: the parser must not read them (they are not in the stream)
                Pw = P.copy()
                for k, o in enumerate(mts.abi.BSDF_COLOR_SLOTS[btype]):
                    if arg[k] is not None: Pw[o:o + 3] = 0.123
                s = W.Stream(prec); WT.bsdf(s, "b", btype, Pw, slot_tex, mask, twosided=two, tex_parent=tex_parent)
                rc, msg, t, B, m, st, tex, own = _parse(sp, mts, s.bytes(), prec)
                assert rc == 0 and own == 0 and len(t) == 1, msg
                assert int(t[0]) == (btype | (0x100 if two else 0)) and m.tolist() == [mask]
                assert np.array_equal(B[0].view(np.uint32), P.view(np.uint32)), (btype, pick, B[0], P)
                want = [a for a in slot_tex if a is not None]
                assert len(tex) == len(want) and all(_same(d, a) for d, a in zip(tex, want)), (btype, pick)
                assert [(-1 if k < 0 else want[k].kind) for k in st[0]] == [(-1 if a is None else a.kind) for a in slot_tex]
                assert [k for k in st[0] if k >= 0] == list(range(len(want))) and [(-1 if a is None else 0) for a in slot_tex] == [min(k, 0) for k in row]


def test_refusals(sp, mts, tmp_path_factory):
    check, grid = _textures(mts)
    P = _block(mts, 5, check, check)[0]
    s = W.Stream(); WT.bsdf(s, "b", 5, P, (check, check), share=True)
    rc, msg, t, B, m, st, tex, own = _parse(sp, mts, s.bytes())
    assert rc == 1 and len(t) == 0 and len(tex) == 0 and "Checkerboard instance shared with another slot" in msg, msg
    G = _block(mts, 6, 0.5, 0.5)[0]
    for a in (check, grid):
        s = W.Stream(); WT.bsdf(s, "b", 6, G, alpha_tex=a)
        rc, msg, *_ = _parse(sp, mts, s.bytes())
        assert rc == 1 and "alpha of RoughGlass is a " + WT.CLASS_OF_KIND[a.kind] + " texture" in msg and "float texture" in msg, msg
    # a composite child with a textured slot, named by its number; the same children with constants are fine
    L = _block(mts, 0, 0.5, None)[0]
    for slot_tex, ok in (((None, None), True), ((None, grid), False)):
        s = W.Stream(); WT.composite(s, "c", [0.4, 0.6], [(("k", 0), 0, L, (None, None)), (("k", 1), 5, P, slot_tex)])
        rc, msg, t, B, m, st, tex, own = _parse(sp, mts, s.bytes())
        if ok:
            assert rc == 0 and own == 2 and st.tolist() == [[-1, -1]] * 3 and not tex, msg
        else:
            assert rc == 1 and len(t) == 0 and len(st) == 0 and not tex and "child 1 (Phong) has a uv texture" in msg, msg
    # truncated inside the texture object: every cut is reported, nothing is handed out
    s = W.Stream(); WT.bsdf(s, "b", 0, L, (grid, None))
    good = s.bytes()
    for cut in (1, 3, 4, 9, 17, 30, 44):
        rc, msg, t, B, m, st, tex, own = _parse(sp, mts, good[:-cut])
        assert rc == 1 and "end of the serialized stream" in msg and not tex, (cut, msg)
    # a caller that takes no textures (the vertex-colour harness) is refused as before
    vc = _build(tmp_path_factory.mktemp("harness_vcol2"), "libstreamharness_vcol.so", "harness_vcol.cpp")
    data = good; buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
    msgb = C.create_string_buffer(512)
    assert vc.sp_parse_bsdf_table_plain(buf, C.c_size_t(len(data)), 4, msgb, C.c_size_t(512)) == 1
    assert "is a GridTexture; only constant reflectances are supported" in msgb.value.decode()
