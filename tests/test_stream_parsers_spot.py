"""integration/streamparse.h and the spot luminaire's projection texture, on bytes: streams written by
tests/mts_stream_writer_spot.py in both precisions -> the block parseSpot gives and the texture description
mtsgpu_set_spot_textures takes: every texture class, all three filter types and four wrap modes, the refused classes, every prefix
of one stream and a few hundred corrupted copies (a refusal or a parse, never a crash: the harness is built with the
undefined-behaviour sanitizer), and the old parseSpot still refusing what it refused."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_bmp as WB
import mts_stream_writer_spot as WS
import spot_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAYLOAD = bytes(range(37))


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_spot") / "libstreamharness_spot.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_spot.cpp"), "-o", so])
    return C.CDLL(so)


def _parse(sp, data, prec=4, plain=False):
    P = np.full(32, 7.0, dtype=np.float32)
    tex = np.zeros(12, dtype=np.uint32); info = np.zeros(8, dtype=np.uint64); gamma = C.c_float(0)
    msg = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    if plain:
        rc = sp.sp_parse_spot_plain(buf, C.c_size_t(len(data)), prec, P.ctypes.data_as(C.POINTER(C.c_float)), msg, C.c_size_t(512))
    else:
        rc = sp.sp_parse_spot_textured(buf, C.c_size_t(len(data)), prec, P.ctypes.data_as(C.POINTER(C.c_float)), tex.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       info.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(gamma), msg, C.c_size_t(512))
    return rc, msg.value.decode(errors="replace"), P, tex, info, gamma.value


def _stream(spot, tex, prec=4):
    P = spot.block
    w2l = np.eye(4); w2l[:3, :3] = P[10:19].reshape(3, 3); w2l[:3, 3] = -(P[10:19].reshape(3, 3).astype(np.float64) @ P[3:6].astype(np.float64))
    l2w = np.eye(4); l2w[:3, :3] = P[10:19].reshape(3, 3).T; l2w[:3, 3] = P[3:6]
    s = W.Stream(prec)
    WS.spot(s, "l", w2l, l2w, P[0:3], P[19], P[8], tex)
    return s.bytes()


def _same_block(P, want):
    """what the stream carries exactly: intensity, position, the angles and the matrix; the cosines come from this machine's cos"""
    for a, b in ((0, 6), (8, 9), (10, 20)):
        assert np.array_equal(P[a:b].view(np.uint32), want[a:b].view(np.uint32)), (a, P[a:b], want[a:b])
    assert np.allclose(P[6:8], want[6:8], rtol=1e-6)


@pytest.mark.parametrize("prec", [4, 8])
def test_every_texture_class_filter_type_and_wrap_mode(sp, mts, prec):
    spots = SC.spots(mts)
    A = mts.abi
    # a constant texture of any value is the plain spot: falloffCurve never evaluates it (spot.cpp:95)
    for rgb in ((1.0, 1.0, 1.0), (0.5, 0.25, 2.0)):
        rc, msg, P, tex, info, _ = _parse(sp, _stream(spots[1], ("constant", rgb), prec), prec)
        assert rc == 0 and info[0] == 0, msg
        _same_block(P, spots[1].block)
    for k, spot in enumerate(spots[:4]):
        t = WS.Proc(k % 2, 0.25, -0.5, 4.0, -3.0, (1.0, 0.5, 0.25), (0.125, 0.0625, 0.5), 0.07)
        rc, msg, P, tex, info, _ = _parse(sp, _stream(spot, t, prec), prec)
        assert rc == 0 and info[0] == 1 and info[1] == 0 and info[2] == 0, msg
        _same_block(P, spot.block)
        assert tex[0] == (A.TEX_GRID if k % 2 else A.TEX_CHECKERBOARD)
        want = [0.25, -0.5, 4.0, -3.0, 1.0, 0.5, 0.25, 0.125, 0.0625, 0.5] + ([0.07] if k % 2 else [0.0])
        assert np.array_equal(tex[1:12].view(np.float32), np.float32(want))
    wrap_of = {WB.REPEAT: A.WRAP_REPEAT, WB.BLACK: A.WRAP_BLACK, WB.WHITE: A.WRAP_WHITE, WB.CLAMP: A.WRAP_CLAMP}
    for filt, flag in ((WB.EWA, 1), (WB.TRILINEAR, 1), (WB.NONE, 0)):
        for wrap, want_wrap in wrap_of.items():
            t = WB.Ldr(PAYLOAD, gamma=2.2, fmt=WB.JPEG, filter_type=filt, wrap=wrap, uoffset=0.5, vscale=-2.0)
            data = _stream(spots[2], t, prec)
            rc, msg, P, tex, info, gamma = _parse(sp, data, prec)
            assert rc == 0 and info[0] == 1 and info[1] == 1, msg
            assert (info[2], info[3], info[4], info[5], info[7]) == (flag, want_wrap, filt, WB.JPEG, len(PAYLOAD)) and gamma == np.float32(2.2)
            assert data[int(info[6]):int(info[6]) + int(info[7])] == PAYLOAD and tex[0] == A.TEX_BITMAP
            assert np.array_equal(tex[1:5].view(np.float32), np.float32([0.5, 0.0, 1.0, -2.0]))
            _same_block(P, spots[2].block)
            # the old parser keeps refusing it
            rc, msg = _parse(sp, data, prec, plain=True)[:2]
            assert rc != 0 and "projection textures of spot luminaires are not on this path" in msg


def test_refused_classes_and_fields(sp, mts):
    spot = SC.spots(mts)[0]
    for cls in ("ExrTexture", "VertexColors", "ScaleTexture"):
        rc, msg = _parse(sp, _stream(spot, ("other", cls)))[:2]
        assert rc != 0 and ("is a " + cls) in msg, msg
        assert ("out of scope" in msg) == (cls != "ScaleTexture")
    rc, msg = _parse(sp, _stream(spot, WB.Ldr(PAYLOAD, filter_type=3)))[:2]
    assert rc != 0 and "unknown filter type 3" in msg
    rc, msg = _parse(sp, _stream(spot, WB.Ldr(PAYLOAD, wrap=4)))[:2]
    assert rc != 0 and "unknown wrap mode 4" in msg
    rc, msg = _parse(sp, _stream(spot, WB.Ldr(PAYLOAD, declared_size=10 ** 6)))[:2]
    assert rc != 0 and "truncated" in msg
    s = W.Stream(); W.directional(s, "l", np.eye(4), np.eye(4), (0, 0, 1), (1, 1, 1), (0, 0, 0), 1.0)
    rc, msg = _parse(sp, s.bytes())[:2]
    assert rc != 0 and "expected a SpotLuminaire" in msg
    # the old parser on what it always refused, and on what it always took
    rc, msg = _parse(sp, _stream(spot, ("constant", (0.5, 0.5, 0.5))), plain=True)[:2]
    assert rc != 0 and "projection textures of spot luminaires are not on this path" in msg
    rc, msg, P = _parse(sp, _stream(spot, ("constant", (1.0, 1.0, 1.0))), plain=True)[:3]
    assert rc == 0
    _same_block(P, spot.block)


def test_prefixes_and_corrupted_copies_never_crash(sp, mts):
    spot = SC.spots(mts)[5]
    data = _stream(spot, WB.Ldr(PAYLOAD, filter_type=WB.EWA, wrap=WB.CLAMP))
    for n in range(len(data)):
        rc, msg = _parse(sp, data[:n])[:2]
        assert rc != 0 and msg, n
    assert _parse(sp, data)[0] == 0
    rng = np.random.RandomState(8)
    parsed = refused = 0
    for streams in (data, _stream(spot, WS.Proc(1))):
        for _ in range(200):
            b = bytearray(streams)
            for _ in range(rng.randint(1, 4)):
                b[rng.randint(len(b))] = rng.randint(256)
            rc, msg = _parse(sp, bytes(b))[:2]
            parsed += rc == 0; refused += rc != 0
            assert rc == 0 or msg
    assert parsed > 0 and refused > 0
