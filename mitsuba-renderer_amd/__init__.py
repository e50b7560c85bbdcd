"""mitsuba-renderer_amd: MI355X-native path-tracing hot path behind Mitsuba 0.2.1's
integrator interface.

Host-side mirror of the reference's objects for this path, over the C ABI of
include/mtsgpu.h (libmtsgpu.so, built by csrc/Makefile):

    Scene          <- Scene + ShapeKDTree after Scene::initialize()   (src/librender/scene.cpp:291-332)
    PerspectiveCamera  <- PerspectiveCameraImpl                      (src/cameras/perspective.cpp)
    MIPathTracer   <- the `path` integrator plugin                   (src/integrators/path/path.cpp)

There is no CPU fallback: every compute call raises if libmtsgpu.so or a gfx950
device is missing.  (The CPU oracle lives in oracle/ and is test infrastructure.)

This file only gathers the names: binding.py loads and builds the library and holds the table of its signatures,
flatscene.py the flattened Scene and its upload plan, cameras.py the cameras, drivers.py the integrators and the device
group, hooks.py the read-outs for tests and measurements."""
from . import abi, binding, scenes, filmreduce, testmode  # noqa: F401
from .testmode import write_mfile, analyze  # noqa: F401
from .scenes import load_weave, Weave, Yarn  # noqa: F401
from .binding import (LIB_PATH, EXPORTS, MASK_EXPORTS, SNOW_EXPORTS, CLOTH_EXPORTS, SPOT_EXPORTS, CYLINDER_EXPORTS, MtsGpuError,  # noqa: F401
                      sources, source_hash, built_hash, _probe_hash, _make_jobs, build, lib)
from .flatscene import (Scene, load_serialized, snow_configure, bsdf_mask_array, bsdf_snow_array, weave_array, uv_texture_array,  # noqa: F401
                        bitmap_array, bitmap_table)
from .cameras import PerspectiveCamera, OrthographicCamera  # noqa: F401
from .hooks import (DEVMATH, cloth_check, devmath, spot_textures_check, ldr_texels, cylinder_configure, cylinder_aabb, cylinder_clip,  # noqa: F401
                    sky_configure, hbm_triad_gbs, gather_roof)
from .drivers import MIPathTracer, MIDirectIntegrator, DeviceGroup, develop  # noqa: F401
