"""integration/streamparse.h and the `mask` BSDF, on bytes: streams written by tests/mts_stream_writer_mask.py with a Mask around
every class, plain and under the twosided adapter, with each opacity source (a constant, a checkerboard, a grid texture, an
unfiltered LDRTexture) -> the nested BSDF's entry with the mask next to it; every refusal (a Mask inside a Mask, as a composite's
child, under TwoSidedBRDF, around a Composite, a VertexColors opacity, a filtered LDRTexture, a missing nested BSDF); and a
caller without the list, who is refused as before."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_bmp as WB
import mts_stream_writer_mask as WM
import mts_stream_writer_ward as WW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, CONSTANT, TEXTURE = 0, 1, 2


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_mask") / "libstreamharness_mask.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_mask.cpp"), "-o", so])
    return C.CDLL(so)


class Parsed:
    pass


def _parse(sp, mts, data, prec=4, with_masks=1, cap=16):
    types = np.zeros(cap, dtype=np.uint32); params = np.zeros((cap, 16), dtype=np.float32); slots = np.zeros(cap, dtype=np.uint32)
    slot_tex = np.zeros((cap, 2), dtype=np.int32); mask_ints = np.full((cap, 3), -9, dtype=np.int32); opacity = np.zeros((cap, 3), dtype=np.float32)
    tex = (mts.abi.UvTexture * cap)(); bmp_tex = np.zeros(cap, dtype=np.int32)
    n, nt, nb, own = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(768)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    u32p, i32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)
    o = Parsed()
    o.rc = sp.sp_parse_bsdf_table_mask(buf, C.c_size_t(len(data)), prec, with_masks, types.ctypes.data_as(u32p), params.ctypes.data_as(f32p),
                                       slots.ctypes.data_as(u32p), slot_tex.ctypes.data_as(i32p), mask_ints.ctypes.data_as(i32p),
                                       opacity.ctypes.data_as(f32p), cap, C.byref(n), tex, cap, C.byref(nt), bmp_tex.ctypes.data_as(i32p), C.byref(nb),
                                       C.byref(own), msg, C.c_size_t(768))
    o.msg, o.own, o.n = msg.value.decode(errors="replace"), own.value, n.value
    o.types, o.params, o.slot_tex, o.tex = types[:n.value], params[:n.value], slot_tex[:n.value], list(tex[:nt.value])
    o.kind, o.texture, o.reserved, o.opacity = mask_ints[:n.value, 0], mask_ints[:n.value, 1], mask_ints[:n.value, 2], opacity[:n.value]
    o.bmp_texture = bmp_tex[:nb.value].tolist()
    return o


def _blocks(mts):
    """[(table type, block)] for the classes 0..8"""
    sd = mts.scenes.SceneDescription("b")
    ids = [sd.lambertian(0.5, 0.6, 0.4), sd.dielectric(1.4, 1.1), sd.roughmetal(0.3), sd.microfacet(0.2), sd.mirror(0.7), sd.phong(15.0, 0.4, 0.3),
           sd.roughglass(0.2), sd.difftrans(0.6), sd.ward(0.15, 0.3)]
    return [(sd.bsdf_type[i], sd.bsdf_params[i]) for i in ids]


def _stream(prec, key, opacity, nested):
    s = W.Stream(prec)
    WM.mask(s, key, opacity, nested)
    return s.bytes()


@pytest.mark.parametrize("prec", [4, 8])
def test_a_mask_around_every_class(sp, mts, prec):
    op = np.float32([0.25, 0.5, 0.75])
    for btype, P in _blocks(mts):
        for two in (0, 0x100):
            o = _parse(sp, mts, _stream(prec, "m", op, WM.any_bsdf("n", btype | two, P)), prec)
            assert o.rc == 0 and o.own == 0 and o.n == 1, (btype, two, o.msg)
            assert o.types[0] == btype | two and np.array_equal(o.params[0].view(np.uint32), P.view(np.uint32)), (btype, two)
            assert (o.kind[0], o.texture[0], o.reserved[0]) == (CONSTANT, -1, 0) and np.array_equal(o.opacity[0], op)
            assert o.slot_tex.tolist() == [[-1, -1]] and not o.tex


def test_each_opacity_source(sp, mts):
    S = mts.scenes
    btype, P = _blocks(mts)[5]
    nested = lambda: WM.any_bsdf("n", btype, P)
    check = S.Checkerboard(bright=(0.9, 0.8, 0.7), dark=(0.2, 0.4, 0.6), uscale=3.0, voffset=0.25)
    o = _parse(sp, mts, _stream(4, "m", check, nested()))
    assert o.rc == 0 and (o.kind[0], o.texture[0]) == (TEXTURE, 0) and len(o.tex) == 1 and o.tex[0].kind == 0, o.msg
    assert np.array_equal(o.opacity[0], np.float32([0.2, 0.4, 0.6]) * np.float32(0.5)), "getAverage() of a checkerboard"
    assert (o.tex[0].uscale, o.tex[0].voffset) == (3.0, 0.25) and o.slot_tex.tolist() == [[-1, -1]], "the mask's texture sits in no slot"
    grid = S.GridTexture(bright=(0.9, 0.8, 0.7), dark=0.1, line_width=0.05)
    o = _parse(sp, mts, _stream(4, "m", grid, nested()))
    assert o.rc == 0 and (o.kind[0], o.texture[0]) == (TEXTURE, 0) and o.tex[0].kind == 1 and np.array_equal(o.opacity[0], np.float32([0.9, 0.8, 0.7]))
    ldr = WB.Ldr(b"\0\xff" * 40, "leaf.png", wrap=WB.CLAMP)
    o = _parse(sp, mts, _stream(4, "m", ldr, nested()))
    assert o.rc == 0 and (o.kind[0], o.texture[0]) == (TEXTURE, 0) and o.tex[0].kind == 2 and o.bmp_texture == [0], o.msg
    assert not o.opacity[0].any(), "the caller decodes the file and writes getAverage()"
    # the mask's texture is read first; the nested BSDF's own slot texture follows it in the list
    s = W.Stream()
    WM.mask(s, "m", check, lambda s: WB.bsdf(s, "n", 0, P, slot_tex=(grid, None)))
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.texture[0] == 0 and o.slot_tex.tolist() == [[1, -1]] and [t.kind for t in o.tex] == [0, 1], o.msg
    # mask(twosided(x)) exists in the reference; the nested block is what the class alone gives
    o = _parse(sp, mts, _stream(4, "m", (0.5, 0.5, 0.5), WM.any_bsdf("n", btype | 0x100, P)))
    assert o.rc == 0 and o.types[0] == btype | 0x100


def test_entries_without_a_mask_get_none(sp, mts):
    blocks = _blocks(mts)
    s = W.Stream(); WW.any_bsdf(s, "b", blocks[0][0], blocks[0][1])
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.kind.tolist() == [NONE] and o.texture.tolist() == [-1] and not o.opacity.any()
    s = W.Stream(); WW.composite(s, "c", [0.5, 0.5], [("a", 0, blocks[0][1]), ("b", 8, blocks[8][1])])
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.own == 2 and o.kind.tolist() == [NONE] * 3 and o.texture.tolist() == [-1] * 3


def test_refusals(sp, mts):
    S = mts.scenes
    blocks = _blocks(mts)
    lam = WM.any_bsdf("n", 0, blocks[0][1])
    half = (0.5, 0.5, 0.5)

    def refused(data, *words, **kw):
        o = _parse(sp, mts, data, **kw)
        assert o.rc == 1 and o.own == -1 and o.n == 0 and not o.tex and not o.bmp_texture, o.msg
        for w in words:
            assert w in o.msg, (w, o.msg)
        return o.msg
    inner = lambda s: WM.mask(s, "inner", half, WM.any_bsdf("n2", 0, blocks[0][1]))
    refused(_stream(4, "m", half, inner), "a Mask inside a Mask")
    s = W.Stream(); WM.composite("c", [0.5, 0.5], [lam, lambda s: WM.mask(s, "m", half, WM.any_bsdf("n2", 5, blocks[5][1]))])(s)
    refused(s.bytes(), "Composite: child 1 is a Mask")
    s = W.Stream(); WM.twosided(s, "t", lambda s: WM.mask(s, "m", half, lam))
    refused(s.bytes(), "a Mask under TwoSidedBRDF", "twosided.cpp:71-73")
    comp = WM.composite("c", [0.5, 0.5], [lam, WM.any_bsdf("n2", 8, blocks[8][1])])
    refused(_stream(4, "m", half, comp), "a Mask around a Composite")
    refused(_stream(4, "m", half, lambda s: WM.twosided(s, "t", comp)), "a Mask around a Composite")
    refused(_stream(4, "m", WM.VERTEX_COLORS, lam), "opacity of Mask is a VertexColors texture", "not supported")
    for ft, name in ((WB.EWA, "ewa"), (WB.TRILINEAR, "trilinear")):
        refused(_stream(4, "m", WB.Ldr(b"abc", filter_type=ft), lam), "opacity of Mask is an LDRTexture with filterType \"%s\"" % name, "ray differentials")
    refused(_stream(4, "m", half, None), "Mask: a nested BSDF is missing")
    refused(_stream(4, "m", None, lam), "opacity of Mask is missing")
    refused(_stream(4, "m", half, lam)[:-7], "")
    # a failure takes back the texture the opacity had appended
    refused(_stream(4, "m", S.Checkerboard(), inner), "a Mask inside a Mask")
    # without the list a Mask is what it was: a class that is not on this path, whatever is inside
    for data in (_stream(4, "m", half, lam), _stream(4, "m", S.Checkerboard(), lam)):
        msg = refused(data, "BSDF class Mask is not on this path", with_masks=0)
        assert "while reading a Mask" in msg
    s = W.Stream(); WM.twosided(s, "t", lambda s: WM.mask(s, "m", half, lam))
    refused(s.bytes(), "BSDF class Mask is not on this path", with_masks=0)
