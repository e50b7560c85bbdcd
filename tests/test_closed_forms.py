"""The oracle's BSDFs and delta luminaires against tests/ref64.py, the binary64 restatement of the reference's shading
formulas (the same cases run against the device in test_gpu_closed_forms.py)."""
import numpy as np
import pytest

import closed_forms as cf
import ref64


@pytest.fixture(scope="module")
def models(mts):
    return cf.parameter_sets(mts)


@pytest.mark.parametrize("index", range(27))
def test_oracle_bsdf_against_binary64(orc, models, index):
    """f, pdf and sample of one model: exact zeros where the reference has them, values within K_VALUE eps cond,
    sampled directions and types, the weight of a sample at the oracle's own direction"""
    name, btype, params = models[index]
    failures, report = cf.check_model(orc.bsdf_eval, name, btype, params, np.random.RandomState(300 + index))
    assert not failures, "\n".join(failures) + "\nworst ratios: %s" % report


def test_parameter_list_is_complete(models):
    assert len(models) == 27


def _poisoned(evaluate, op_hit, cols):
    """evaluate, with a NaN written into the given output columns of every third nonzero record of one op"""
    def ev(btype, params, op, wi, aux):
        out = evaluate(btype, params, op, wi, aux)
        if op == op_hit:
            rows = np.nonzero((out[:, cols] != 0).any(axis=1))[0][::3]
            out[np.ix_(rows, cols)] = np.nan
        return out
    return ev


@pytest.mark.parametrize("op,cols", [(0, [0, 1, 2]), (0, [1]), (1, [0]), (2, [3]), (2, [4, 5, 6]), (2, [0, 1, 2])])
def test_nan_results_fail_the_checks(orc, models, op, cols):
    """the checks must see a NaN where the reference is finite: f, pdf, a sample's pdf, weight or direction"""
    for index in (0, 3, 5, 6):
        name, btype, params = models[index]
        failures, report = cf.check_model(_poisoned(orc.bsdf_eval, op, cols), name, btype, params,
                                          np.random.RandomState(300 + index))
        assert failures, (name, op, cols, report)


def test_nan_pixels_fail_the_render_check(mts, orc):
    name, sd, b, light, integ = cf.render_cases(mts)[0]
    cam = orc.make_camera(sd, cf.W, cf.H)
    fs = orc.FlatScene(sd)                 # keeps the flattened scene alive while it renders
    film, _ = orc.render(fs.scene, cam, orc.render_params(2, spp=cf.SPP, seed=7, integrator=integ))
    img = orc.develop(film)
    assert not cf.check_render(img, cam, sd.bsdf_type[b], sd.bsdf_params[b], light)[0]
    for value in (np.nan, np.inf):
        bad = img.copy()
        bad[img > 0] = value
        assert cf.check_render(bad, cam, sd.bsdf_type[b], sd.bsdf_params[b], light)[0]
    bad = img.copy(); bad[5, 7, 1] = np.nan
    assert cf.check_render(bad, cam, sd.bsdf_type[b], sd.bsdf_params[b], light)[0]


@pytest.mark.parametrize("distr", [0, 1, 2])
def test_oracle_index_matched_roughglass(orc, distr):
    cf.assert_index_matched_roughglass(orc.bsdf_eval, distr)


@pytest.mark.parametrize("index", range(10))
def test_oracle_delta_light_renders(mts, orc, index):
    name, sd, b, light, integ = cf.render_cases(mts)[index]
    fs = orc.FlatScene(sd)
    cam = orc.make_camera(sd, cf.W, cf.H)
    film, _ = orc.render(fs.scene, cam, orc.render_params(2, sampler=mts.abi.SAMPLER_INDEPENDENT_KEYED, spp=cf.SPP,
                                                         seed=7, integrator=integ))
    img = orc.develop(film)
    failures, worst, n_zero, n_lit = cf.check_render(img, cam, sd.bsdf_type[b], sd.bsdf_params[b], light)
    assert not failures, (name, failures, worst)
    assert n_lit > 0 and (n_zero > 0 or name not in ("spot light", "collimated beam"))
