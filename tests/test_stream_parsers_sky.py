"""The reader of integration/streamparse.h for SkyLuminaire::serialize on bytes: streams written by
tests/mts_stream_writer_sky.py (an independent writer that follows Luminaire::serialize and SkyLuminaire::serialize) -> a
parameter block that must equal what the library's flattener keeps for the same scene description, bit for bit; both Float
precisions, truncated streams, a stream of another class."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import mts_stream_writer as W
import mts_stream_writer_sky as WS
import sky_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_sky") / "libstreamharness_sky.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_sky.cpp"), "-o", so])
    return C.CDLL(so)


def _parse(sp, data, prec=4):
    P = np.zeros(32, dtype=np.float32)
    msg = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    rc = sp.sp_parse_sky(buf, C.c_size_t(len(data)), prec, P.ctypes.data_as(C.POINTER(C.c_float)), msg, C.c_size_t(512))
    return rc, msg.value.decode(errors="replace"), P


def _m44(M3):
    M = np.eye(4); M[:3, :3] = np.asarray(M3, dtype=np.float64).reshape(3, 3)
    return M


SKIES = [dict(), dict(sun_direction=(0.3, 0.2, 0.8), turbidity=4.0, sky_scale=0.25, clip_below_horizon=False),
         dict(sun_direction=(-0.2, 0.5, 0.4), turbidity=5.0, a=1.3, b=0.7, c=1.5, d=0.8, e=1.2, to_world=sky_cases._rot((1.0, 0.2, 0.4), -115.0))]


def _flattened(mts, kw):
    sd = mts.scenes.SceneDescription("sky stream")
    pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.5), face_normals=True)
    l = sd.sky(**kw)
    return np.array(mts.Scene(sd).arrays()["lum_params"][l], dtype=np.float32)


def _stream(P, prec):
    s = W.Stream(prec)
    w2l = _m44(P[7:16])
    WS.sky(s, "sky", w2l, np.linalg.inv(w2l), P[0], P[1], P[16], P[17], P[18:23], P[2] != 0, name="sky")
    return s.bytes()


@pytest.mark.parametrize("prec", [4, 8])
@pytest.mark.parametrize("k", range(3))
def test_sky_block_from_bytes(sp, mts, prec, k):
    """every field the stream carries lands where the flattener puts it; the bounding sphere [3..6] is not in the stream
    (preprocess() derives it) and stays as the caller left it"""
    F = _flattened(mts, SKIES[k])
    rc, msg, P = _parse(sp, _stream(F, prec), prec)
    assert rc == 0, msg
    assert not P[3:7].any() and F[6] > 0
    P[3:7] = F[3:7]
    assert np.array_equal(P.view(np.uint32), F.view(np.uint32)), (P, F)


@pytest.mark.parametrize("prec", [4, 8])
def test_truncated_streams_fail(sp, mts, prec):
    data = _stream(_flattened(mts, SKIES[1]), prec)
    for cut in (0, 3, 12, len(data) // 2, len(data) - 5, len(data) - 1):
        rc, msg, _ = _parse(sp, data[:cut], prec)
        assert rc == 1 and "unexpected end" in msg, (cut, msg)
    assert _parse(sp, data, prec)[0] == 0


def test_another_class_is_refused(sp, mts):
    s = W.Stream(4)
    W.collimated(s, "c", np.eye(4), np.eye(4), (1.0, 1.0, 1.0), 0.1)
    rc, msg, _ = _parse(sp, s.bytes())
    assert rc == 1 and "expected a SkyLuminaire" in msg
