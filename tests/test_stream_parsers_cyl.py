"""integration/streamparse.h and the cylinder, on bytes: streams written by tests/mts_stream_writer_cyl.py with a Cylinder behind
Shape::serialize, in both precisions -> the derived block of include/mtsgpu_cylinder.h, equal to the flattener's bit for bit; a
nested BSDF of every class the parser skips from the end; a nested area luminaire (refused with the library's reason); truncated
and corrupted streams."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import cyl_cases as CC
import mts_stream_writer as W
import mts_stream_writer_cyl as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sp(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("harness_cyl") / "libstreamharness_cyl.so")
    subprocess.check_call(["g++", "-std=gnu++11", "-O1", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-shared",
                           "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "integration"),
                           os.path.join(ROOT, "tests", "stream_harness", "harness_cyl.cpp"), "-o", so])
    return C.CDLL(so)


def _parse(sp, data, prec=4, is_luminaire=0):
    D = np.full(28, 7.0, dtype=np.float32)
    msg = C.create_string_buffer(512)
    buf = (C.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    rc = sp.sp_parse_cylinder(buf, C.c_size_t(len(data)), prec, is_luminaire, D.ctypes.data_as(C.POINTER(C.c_float)), msg, C.c_size_t(512))
    return rc, msg.value.decode(errors="replace"), D


def _blocks(mts):
    out = [mts.cylinder_configure(mts.scenes.CylinderDesc(p1, p2, r)) for _, p1, p2, r in CC.POSES]
    return out + [mts.cylinder_configure(mts.scenes.CylinderDesc(to_world=CC.SHEARED))]


def _write(block, prec, **kw):
    o2w = np.eye(4, dtype=np.float32); o2w[:3] = block[0:12].reshape(3, 4)
    w2o = np.eye(4, dtype=np.float32); w2o[:3] = block[12:24].reshape(3, 4)
    s = W.Stream(prec)
    WC.cylinder(s, ("shape", 0), o2w, w2o, block[24], block[25], **kw)
    return s.bytes()


def _bsdfs(mts):
    """one (type, block, twosided) per BSDF class of the test scenes: what sits between the shape's header and the cylinder's tail"""
    out = []
    for sd in (mts.scenes.cornell_c5(), mts.scenes.spheres()):
        fa = mts.Scene(sd).arrays()
        for t, p in zip(fa["bsdf_type"], fa["bsdf_params"]):
            if (int(t) & 0xFF) not in [a[0] for a in out]:
                out.append((int(t) & 0xFF, np.array(p, dtype=np.float32), bool(int(t) & mts.abi.BSDF_TWOSIDED)))
    return out


@pytest.mark.parametrize("prec", [4, 8])
def test_cylinder_from_bytes_equals_the_flattener(sp, mts, prec):
    bsdfs = _bsdfs(mts)
    assert len(bsdfs) >= 5
    for k, block in enumerate(_blocks(mts)):
        for bargs in [None] + bsdfs:
            rc, msg, g = _parse(sp, _write(block, prec, bsdf_args=bargs), prec)
            assert rc == 0, msg
            if prec == 4:
                assert np.array_equal(g.view(np.uint32), block.view(np.uint32)), (k, g, block)
            else:
                # the binary32 fields are exact in binary64; 1 / area is formed in binary64 there and rounded once
                assert np.array_equal(g[:26].view(np.uint32), block[:26].view(np.uint32)) and np.isclose(g[26], block[26], rtol=2e-7) and g[27] == 0
    # the same block from the scene flattener (the pool next to the scene)
    sd = CC.scene_description(mts, "mixed")
    pool = mts.Scene(sd).cylinder_blocks()
    rc, msg, g = _parse(sp, _write(pool[0], 4, bsdf_args=bsdfs[0]), 4)
    assert rc == 0 and np.array_equal(g.view(np.uint32), pool[0].view(np.uint32))


@pytest.mark.parametrize("prec", [4, 8])
def test_nested_luminaire_is_refused_and_skipped(sp, mts, prec):
    block = _blocks(mts)[1]
    data = _write(block, prec, bsdf_args=_bsdfs(mts)[0], lum_intensity=(1.0, 2.0, 3.0))
    rc, msg, _ = _parse(sp, data, prec, is_luminaire=1)
    assert rc != 0 and "pdfArea" in msg and "area luminaire" in msg
    # the nested luminaire itself is skipped like the BSDF: the tail is read from the end
    rc, msg, g = _parse(sp, data, prec, is_luminaire=0)
    assert rc == 0 and np.array_equal(g[:26].view(np.uint32), block[:26].view(np.uint32))


def test_truncated_corrupted_and_foreign_streams(sp, mts):
    block = _blocks(mts)[1]
    data = _write(block, 4, bsdf_args=_bsdfs(mts)[0])
    tail = 2 * 16 * 4 + 2 * 4
    answers = set()
    for n in range(len(data)):
        rc, msg, _ = _parse(sp, data[:n], 4)
        answers.add(rc)
        if n < tail + 8:
            assert rc != 0 and msg, n                  # shorter than the tail behind the class name: never a block
    assert answers <= {0, 1}
    rc, msg, _ = _parse(sp, b"", 4)
    assert rc != 0
    rng = np.random.RandomState(2)
    for _ in range(300):
        bad = bytearray(data)
        for i in rng.randint(0, len(bad), size=rng.randint(1, 6)):
            bad[i] = rng.randint(0, 256)
        rc, msg, g = _parse(sp, bytes(bad), 4)
        assert rc in (0, 1) and (rc == 0 or msg)
    # a last row that is not 0 0 0 1
    o2w = np.eye(4, dtype=np.float32); o2w[3, 2] = 0.5
    s = W.Stream(4); WC.cylinder(s, "c", o2w, np.eye(4), 1.0, 1.0)
    rc, msg, _ = _parse(sp, s.bytes(), 4)
    assert rc != 0 and "affine" in msg
    # another class under the cylinder's parser
    s = W.Stream(4); W.sphere(s, "s", np.eye(4), np.eye(4), 1.0, (0, 0, 0), False)
    rc, msg, _ = _parse(sp, s.bytes(), 4)
    assert rc != 0 and "Cylinder" in msg
