"""Writer for the object stream of the sky luminaire of Mitsuba 0.2.1, next to tests/mts_stream_writer.py (whose Stream and
Luminaire::serialize it uses): it follows SkyLuminaire::serialize.  Test infrastructure; nothing here is used by the product."""
import mts_stream_writer as W


def sky(s, key, w2l, l2w, sky_scale, turbidity, theta_s, phi_s, consts, clip_below_horizon, name=""):
    """SkyLuminaire::serialize (src/luminaires/sky.cpp:121-133) behind Luminaire::serialize (src/librender/luminaire.cpp:66-74):
    skyScale, turbidity, thetaS, phiS, aConst .. eConst as Floats, clipBelowHorizon as a bool (one byte).  The object is
    written detached (no parent), its type is the base class's default, it is not intersectable."""
    def body(s):
        W.luminaire_base(s, w2l, l2w, ltype=0, intersectable=False, name=name)
        s.float(sky_scale); s.float(turbidity); s.float(theta_s); s.float(phi_s)
        for c in consts:
            s.float(c)
        s.bool(clip_below_horizon)
    s.ref(key, "SkyLuminaire", body)
