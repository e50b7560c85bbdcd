"""integration/streamparse.h and the `ldrtexture` texture, on bytes: streams written by tests/mts_stream_writer_bmp.py with an
LDRTexture in each slot of each class -> its descriptor (kind MTSGPU_TEX_BITMAP) in the texture list, its fields and the span
of its encoded file in the bitmap list, offset and size exact over an arbitrary payload; what is refused (ewa, trilinear, a
shared instance, a float slot, a truncated payload, a composite child, a caller without the list); a table that mixes a
checkerboard and a bitmap.  Nothing is decoded: the parser has no image decoder, the plugin has Mitsuba's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_bmp as WB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = [0, 1, 2, 3, 5, 6, 7, 8]            # Mirror keeps a plain Spectrum (mirror.cpp:51-55): no texture to replace
WRAP_OF = {WB.REPEAT: 0, WB.CLAMP: 1, WB.BLACK: 2, WB.WHITE: 3}      # MIPMap::EWrapMode -> MTSGPU_WRAP_*


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_bmp") / "libstreamharness_bmp.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_bmp.cpp"), "-o", so])
    return C.CDLL(so)


class Parsed:
    pass


def _parse(sp, mts, data, prec=4, with_bitmaps=1, cap=16):
    types = np.zeros(cap, dtype=np.uint32); params = np.zeros((cap, 16), dtype=np.float32); slots = np.zeros(cap, dtype=np.uint32)
    slot_tex = np.zeros((cap, 2), dtype=np.int32)
    tex = (mts.abi.UvTexture * cap)()
    ints = np.zeros((cap, 6), dtype=np.int64); floats = np.zeros((cap, 2), dtype=np.float32); names = C.create_string_buffer(64 * cap)
    n, nt, nb, own = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_int(-2)
    msg = C.create_string_buffer(768)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    u32p = C.POINTER(C.c_uint32)
    o = Parsed()
    o.rc = sp.sp_parse_bsdf_table_bmp(buf, C.c_size_t(len(data)), prec, with_bitmaps, types.ctypes.data_as(u32p), params.ctypes.data_as(C.POINTER(C.c_float)),
                                      slots.ctypes.data_as(u32p), slot_tex.ctypes.data_as(C.POINTER(C.c_int32)), cap, C.byref(n), tex, cap, C.byref(nt),
                                      ints.ctypes.data_as(C.POINTER(C.c_int64)), floats.ctypes.data_as(C.POINTER(C.c_float)), names, C.byref(nb),
                                      C.byref(own), msg, C.c_size_t(768))
    o.msg, o.own = msg.value.decode(errors="replace"), own.value
    o.types, o.params, o.masks, o.slot_tex, o.tex = types[:n.value], params[:n.value], slots[:n.value], slot_tex[:n.value], list(tex[:nt.value])
    o.bmp = [dict(texture=int(ints[k, 0]), format=int(ints[k, 1]), filter=int(ints[k, 2]), wrap=int(ints[k, 3]), offset=int(ints[k, 4]), size=int(ints[k, 5]),
                  gamma=float(floats[k, 0]), aniso=float(floats[k, 1]), name=names.raw[64 * k:64 * k + 64].split(b"\0")[0].decode()) for k in range(nb.value)]
    return o


def _payload(seed, n):
    """arbitrary bytes, zeros and 0xFF among them: the parser must step over them by the declared size alone"""
    p = bytearray(np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes())
    p[:4] = b"\0\0\xff\0"
    return bytes(p)


def _ldrs():
    return (WB.Ldr(_payload(1, 301), "textures/wood.png", -1.0, WB.PNG, WB.NONE, WB.CLAMP, 8.0, 0.3, -0.3, 3.7, -3.7),
            WB.Ldr(_payload(2, 77), "a.jpg", 2.2, WB.JPEG, WB.NONE, WB.WHITE, 4.0, -0.25, 0.5, -2.0, 1.5))


def _block(mts, btype, a, b):
    sd = mts.scenes.SceneDescription("b")
    i = {0: lambda: sd.lambertian(a), 1: lambda: sd.dielectric(1.4, 1.1, refl=a, trans=b), 2: lambda: sd.roughmetal(0.2, 0.4, 2.5, refl=a),
         3: lambda: sd.microfacet(0.15, 0.4, 0.3, 1.6, 1.0, rd=a, rs=b), 5: lambda: sd.phong(17.0, rd=a, rs=b, kd=0.3, ks=0.2),
         6: lambda: sd.roughglass(0.2, 1.5, 1.0, "ggx", refl=a, trans=b), 7: lambda: sd.difftrans(a),
         8: lambda: sd.ward(0.2, 0.2, rd=a, rs=b, kd=0.3, ks=0.2, model="ward-duer")}[btype]()
    return sd.bsdf_params[i]


def _check_bitmap(b, d, ldr, prec):
    f = (lambda v: float(np.float32(v)))
    assert d.kind == 2 and [d.uoffset, d.voffset, d.uscale, d.vscale] == [f(ldr.uoffset), f(ldr.voffset), f(ldr.uscale), f(ldr.vscale)]
    assert list(d.bright) + list(d.dark) + [d.line_width] == [0.0] * 7, "the seven words behind vscale are the library's"
    assert (b["name"], b["format"], b["filter"], b["wrap"]) == (ldr.filename, ldr.fmt, WB.NONE, WRAP_OF[ldr.wrap])
    assert (b["gamma"], b["aniso"]) == (f(ldr.gamma), f(ldr.max_anisotropy))
    assert (b["offset"], b["size"]) == (ldr.offset, len(ldr.payload)), "the span of the encoded file"


@pytest.mark.parametrize("prec", [4, 8])
@pytest.mark.parametrize("btype", TYPES)
def test_ldr_texture_in_every_slot(sp, mts, prec, btype):
    S = mts.scenes
    la, lb = _ldrs()
    check = S.Checkerboard(bright=(0.8, 0.6, 0.4), dark=(0.2, 0.1, 0.3), uoffset=0.3, uscale=3.7)
    offs = mts.abi.BSDF_COLOR_SLOTS[btype]
    n_slots = len(offs)
    assert [sp.sp_bsdf_slot_offset(btype | 0x100, k) for k in range(2)] == [offs[k] if k < n_slots else -1 for k in range(2)]
    choices = [None, la, lb, check]
    for two in (False, True):
        for tex_parent in (False, True):
            for pick in range(len(choices) ** n_slots):
                arg = [choices[(pick // len(choices) ** k) % len(choices)] if k < n_slots else None for k in range(2)]
                if arg[0] is not None and arg[0] is arg[1]:
                    continue                        # one instance in two slots is a refusal, below
                # the block of the mirror with the checkerboard where it is and constants elsewhere; a bitmap's slot comes back 0
                P = _block(mts, btype, *[a if a is check else 0.5 for a in arg])
                Pw, want_P = P.copy(), P.copy()
                for k, o in enumerate(offs):
                    if arg[k] is not None: Pw[o:o + 3] = 0.123      # not in the stream: the parser must not read them
                    if isinstance(arg[k], WB.Ldr): want_P[o:o + 3] = 0.0
                s = W.Stream(prec); WB.bsdf(s, "b", btype, Pw, arg, 0, twosided=two, tex_parent=tex_parent)
                data = s.bytes()
                o = _parse(sp, mts, data, prec)
                assert o.rc == 0 and o.own == 0 and len(o.types) == 1, o.msg
                assert int(o.types[0]) == (btype | (0x100 if two else 0)) and o.masks.tolist() == [0]
                assert np.array_equal(o.params[0].view(np.uint32), want_P.view(np.uint32)), (btype, pick, o.params[0], want_P)
                want = [a for a in arg if a is not None]
                assert len(o.tex) == len(want) and [d.kind for d in o.tex] == [a.kind for a in want]
                assert [k for k in o.slot_tex[0] if k >= 0] == list(range(len(want))) and [(k >= 0) for k in o.slot_tex[0]] == [a is not None for a in arg]
                ldrs = [a for a in want if isinstance(a, WB.Ldr)]
                assert len(o.bmp) == len(ldrs)
                for b, ldr in zip(o.bmp, ldrs):
                    assert want[b["texture"]] is ldr
                    _check_bitmap(b, o.tex[b["texture"]], ldr, prec)
                    assert data[b["offset"]:b["offset"] + b["size"]] == ldr.payload


def test_wrap_modes_are_translated(sp, mts):
    """MIPMap::EWrapMode numbers repeat, black, white, clamp; MTSGPU_WRAP_* repeat, clamp, black, white"""
    L = _block(mts, 0, 0.5, None)
    for wrap, want in WRAP_OF.items():
        s = W.Stream(); WB.bsdf(s, "b", 0, L, (WB.Ldr(b"xyz", wrap=wrap), None))
        o = _parse(sp, mts, s.bytes())
        assert o.rc == 0 and o.bmp[0]["wrap"] == want and o.bmp[0]["size"] == 3, o.msg
    assert [mts.abi.WRAP_REPEAT, mts.abi.WRAP_CLAMP, mts.abi.WRAP_BLACK, mts.abi.WRAP_WHITE] == [WRAP_OF[k] for k in (WB.REPEAT, WB.CLAMP, WB.BLACK, WB.WHITE)]
    s = W.Stream(); WB.bsdf(s, "b", 0, L, (WB.Ldr(b"xyz", wrap=4), None))
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 1 and "unknown wrap mode 4" in o.msg and not o.bmp and not o.tex
    # an empty file is a span of no bytes: the decoder's to refuse
    s = W.Stream(); WB.bsdf(s, "b", 0, L, (WB.Ldr(b""), None))
    o = _parse(sp, mts, s.bytes())
    assert o.rc == 0 and o.bmp[0]["size"] == 0 and o.bmp[0]["offset"] == len(s.bytes()), o.msg


def test_refusals(sp, mts):
    la, lb = _ldrs()
    P = _block(mts, 5, 0.5, 0.5)
    L = _block(mts, 0, 0.5, None)

    def refused(data, **kw):
        o = _parse(sp, mts, data, **kw)
        assert o.rc == 1 and len(o.types) == 0 and not o.tex and not o.bmp and len(o.slot_tex) == 0, o.msg
        return o.msg
    # the filtered modes: the message names the filter, says why and what to set
    for ft, name in ((WB.EWA, "ewa"), (WB.TRILINEAR, "trilinear")):
        s = W.Stream(); WB.bsdf(s, "b", 5, P, (None, WB.Ldr(_payload(3, 40), filter_type=ft)))
        msg = refused(s.bytes())
        assert 'specularReflectance of Phong is an LDRTexture with filterType "%s"' % name in msg and "ray differentials" in msg, msg
        assert 'set filterType to "none"' in msg, msg
    # one instance in two slots
    s = W.Stream(); WB.bsdf(s, "b", 5, P, (la, la), share=True)
    assert "LDRTexture instance shared with another slot" in refused(s.bytes())
    # a float-texture slot
    s = W.Stream(); WB.bsdf(s, "b", 6, _block(mts, 6, 0.5, 0.5), alpha_tex=la)
    msg = refused(s.bytes())
    assert "alpha of RoughGlass is a LDRTexture texture" in msg and "float texture" in msg, msg
    # a payload shorter than its declared size, and every cut of a good stream
    s = W.Stream(); WB.bsdf(s, "b", 0, L, (WB.Ldr(_payload(4, 50), declared_size=51), None))
    assert "encoded file (51 bytes) is truncated" in refused(s.bytes())
    s = W.Stream(); WB.bsdf(s, "b", 0, L, (WB.Ldr(_payload(4, 50), declared_size=0xFFFFFFFF), None))
    assert "encoded file (4294967295 bytes) is truncated" in refused(s.bytes())
    s = W.Stream(); WB.bsdf(s, "b", 0, L, (la, None))
    good = s.bytes()
    assert _parse(sp, mts, good).rc == 0
    for cut in (1, 17, len(la.payload), len(la.payload) + 1, len(la.payload) + 3, len(la.payload) + 9, len(la.payload) + 30, len(la.payload) + 50):
        msg = refused(good[:-cut])
        assert "truncated" in msg or "end of the serialized stream" in msg, (cut, msg)
    # a composite child
    for slot_tex, ok in (((None, None), True), ((None, lb), False)):
        s = W.Stream(); WB.composite(s, "c", [0.4, 0.6], [(("k", 0), 0, L, (None, None)), (("k", 1), 5, P, slot_tex)])
        if ok:
            o = _parse(sp, mts, s.bytes())
            assert o.rc == 0 and o.own == 2 and not o.bmp, o.msg
        else:
            assert "child 1 (Phong) has a uv texture" in refused(s.bytes())
    # a caller that takes uv textures but has not asked for bitmaps is refused as before
    assert "reflectance of Lambertian is a LDRTexture; only constant reflectances are supported" in refused(good, with_bitmaps=0)


def test_table_with_a_checkerboard_and_a_bitmap(sp, mts):
    """one Phong: a grid texture in slot 0, a bitmap in slot 1; then the same parser instance's lists hold both in stream order"""
    S = mts.scenes
    la, _ = _ldrs()
    grid = S.GridTexture(bright=(0.5, 0.25, 0.75), dark=(0.1, 0.05, 0.02), uoffset=-0.3, uscale=-3.7, vscale=2.0, line_width=0.07)
    for prec in (4, 8):
        P = _block(mts, 5, grid, 0.5)
        s = W.Stream(prec); WB.bsdf(s, "b", 5, P, (grid, la), twosided=True)
        o = _parse(sp, mts, s.bytes(), prec)
        assert o.rc == 0 and int(o.types[0]) == 5 | 0x100 and o.slot_tex.tolist() == [[0, 1]], o.msg
        assert [d.kind for d in o.tex] == [1, 2] and o.tex[0].line_width == np.float32(0.07) and list(o.tex[0].bright) == [0.5, 0.25, 0.75]
        assert len(o.bmp) == 1 and o.bmp[0]["texture"] == 1
        _check_bitmap(o.bmp[0], o.tex[1], la, prec)
        want = P.copy(); want[8:11] = 0.0
        assert np.array_equal(o.params[0].view(np.uint32), want.view(np.uint32)) and np.array_equal(o.params[0][5:8], grid.bright)
