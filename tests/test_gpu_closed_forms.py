"""The device's BSDFs (mtsgpu_bsdf_eval, the code k_shade runs) and delta-luminaire renders against tests/ref64.py, the
binary64 restatement of the reference's shading formulas: the cases of test_closed_forms.py, on the MI355X."""
import numpy as np
import pytest

import closed_forms as cf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def models(mts):
    return cf.parameter_sets(mts)


@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer()


@pytest.mark.parametrize("index", range(27))
def test_device_bsdf_against_binary64(device, models, index):
    name, btype, params = models[index]
    failures, report = cf.check_model(device.bsdf_eval, name, btype, params, np.random.RandomState(300 + index))
    assert not failures, "\n".join(failures) + "\nworst ratios: %s" % report


@pytest.mark.parametrize("distr", [0, 1, 2])
def test_device_index_matched_roughglass(device, distr):
    cf.assert_index_matched_roughglass(device.bsdf_eval, distr)


@pytest.mark.parametrize("index", range(10))
def test_device_delta_light_renders(gpu_lib, mts, index):
    name, sd, b, light, integ = cf.render_cases(mts)[index]
    it = mts.MIPathTracer(maxDepth=2) if integ == "path" else mts.MIDirectIntegrator(1, 1)
    cam = mts.PerspectiveCamera.for_description(sd, cf.W, cf.H)
    it.preprocess(mts.Scene(sd), cam, sampler="independent", sampleCount=cf.SPP, seed=7)
    assert it.render()
    img = mts.develop(it.film())
    failures, worst, n_zero, n_lit = cf.check_render(img, cam.c, sd.bsdf_type[b], sd.bsdf_params[b], light)
    assert not failures, (name, failures, worst)
    assert n_lit > 0 and (n_zero > 0 or name not in ("spot light", "collimated beam"))
