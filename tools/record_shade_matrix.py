#!/usr/bin/env python3
"""Prints tests/golden/shade_launch_matrix.json: the SHA-256 of the film of every cell of tests/test_shade_matrix.py, rendered by
the library of this tree on the GPU.  Run it on the commit whose films are the truth, with that commit's library built:

    python tools/record_shade_matrix.py <commit> > tests/golden/shade_launch_matrix.json

The cell list, the scenes and the render are the test's own (imported from tests/test_shade_matrix.py, which may be a copy from a
later commit: it needs nothing but the package and tests/tan_cases.py)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _pkgload  # noqa: E402
import test_shade_matrix as M  # noqa: E402


def main():
    commit = sys.argv[1]
    mts = _pkgload.load()
    films = {}
    for family, sky in M.GROUPS:
        for cell, film in M.render_group(mts, family, sky).items():
            films[cell] = M.film_hash(film)
    doc = {"commit": commit, "command": "python tools/record_shade_matrix.py %s" % commit,
           "library_source_hash": mts.lib().mtsgpu_source_hash().decode(),
           "cells": "family-sky-integrator-driver: %d x %d, %d spp, independent sampler, seed %d, maxDepth %d; sha256 of the film's bytes"
                    % (M.RES, M.RES, M.SPP, M.SEED, M.MAX_DEPTH),
           "films": films}
    json.dump(doc, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
