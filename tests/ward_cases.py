"""The Ward / Composite models that tests/test_ward_composite.py (CPU) and tests/test_gpu_ward_composite.py (device) share:
the two entries of the reference's data/tests/test_bsdf.xml that tests/chisquare_ref.py leaves out, and the edges of their
parameter space.  Test infrastructure."""
import numpy as np

import ref64_ward


def models(mts):
    """[(name, index)] into one scene description's BSDF table, and that description"""
    sd = mts.scenes.SceneDescription("ward and composite")
    out = []
    def add(name, index):
        out.append((name, index))
        return index
    xml_ward = add("test_bsdf.xml ward", sd.ward(0.1, 0.3, rd=1.0, rs=1.0, kd=0.5, ks=0.5))                 # :31-39
    for model in ("ward", "ward-duer", "balanced"):
        add("ward type %s" % model, sd.ward(0.1, 0.1, model=model))
    for a in (0.01, 0.1, 1.0):
        add("ward alpha %g" % a, sd.ward(a, a, rd=0.4, rs=0.6, kd=0.5, ks=0.5))
    add("ward alpha .05 / .5", sd.ward(0.05, 0.5, rd=0.4, rs=0.6, kd=0.5, ks=0.5))
    add("ward specular only", sd.ward(0.1, 0.1, rd=0.0, rs=1.0, kd=0.0, ks=1.0))
    add("ward diffuse only", sd.ward(0.1, 0.1, rd=0.5, rs=0.0, kd=1.0, ks=0.0))
    add("twosided ward", sd.twosided(sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5)))
    phong = sd.phong(20.0, rd=1.0, rs=1.0, kd=0.5, ks=0.5)
    add("test_bsdf.xml composite", sd.composite([0.4, 0.6], [phong, xml_ward]))                              # :55-76
    lam, metal = sd.lambertian(0.5), sd.roughmetal(0.1)
    # lambertian, ward and roughmetal in one composite.  The order is an input of the comparison: closed_forms.sample_inputs
    # puts a fifth of the samples at sample.x = 0 and a fifth at 1 - 2^-24, which sampleReuse hands to the first and the last
    # child at the ends of their own range, and there ref64's roughmetal restatement decides nothing (log(1 - x) at x -> 1,
    # sqrt(x) at x -> 0: its dir_cond is unbounded).  With the metal in the middle the two edge classes reach children whose
    # restatement decides them, and the share of undecidable samples stays under closed_forms.MAX_AMBIGUOUS.
    add("composite lambertian roughmetal ward", sd.composite([0.3, 0.4, 0.3], [lam, metal, xml_ward]))
    add("composite with a zero weight", sd.composite([0.5, 0.0, 0.5], [lam, metal, xml_ward]))
    return out, sd


def evaluator(table):
    """the restatement as a batch evaluator with the layout of mtsgpu_bsdf_eval_table: (index, op, wi, aux) -> [n][8]"""
    def evaluate(index, op, wi, aux):
        t, P = table.types[index], table.params[index]
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = len(aux)
        out = np.zeros((n, 8), dtype=np.float64)
        if op == 0:
            out[:, 0:3] = table.f(t, P, wi, aux)[0]
        elif op == 1:
            out[:, 0] = table.pdf(t, P, wi, aux)[0]
        else:
            r = table.sample(t, P, wi, aux)
            fv = table.f(t, P, wi, r.wo)[0]; pv = table.pdf(t, P, wi, r.wo)[0]
            ok = r.alive
            out[:, 0:3] = np.where(ok[:, None], r.wo, 0.0)
            out[:, 3] = np.where(ok, pv, 0.0)
            out[:, 4:7] = np.where(ok[:, None], fv, 0.0)
        return np.nan_to_num(out, nan=0.0, posinf=0.0, neginf=0.0)
    return evaluate


def table_of(sd):
    return ref64_ward.Table(sd.bsdf_type, sd.bsdf_params)
