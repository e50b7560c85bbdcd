"""Cylinder::serialize (src/shapes/cylinder.cpp:75-80) behind Shape::serialize (src/librender/shape.cpp:130-138), written the way
tests/mts_stream_writer.py writes a sphere: for tests/test_stream_parsers_cyl.py.  Test infrastructure."""
import numpy as np

import mts_stream_writer as W


def cylinder(s, key, o2w, w2o, radius, length, bsdf_args=None, lum_intensity=None, occluder=True):
    eye = np.eye(4)

    def body(s):
        W.configurable(s)                        # the parent (the Scene) was taken off
        if bsdf_args is None: s.ref(None)
        else: W.bsdf(s, (key, "bsdf"), *bsdf_args)
        s.ref(None)                              # m_subsurface
        if lum_intensity is None: s.ref(None)
        else: W.area_luminaire(s, (key, "lum"), key, lum_intensity, eye, eye)
        s.ref(None); s.ref(None)                 # interior / exterior medium
        s.bool(occluder)
        s.transform(o2w, w2o); s.float(radius); s.float(length)
    s.ref(key, "Cylinder", body)
