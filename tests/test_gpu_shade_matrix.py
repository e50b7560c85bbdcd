"""The launch matrix of the shading kernels on the device: every cell of tests/test_shade_matrix.py renders the film whose SHA-256
tests/golden/shade_launch_matrix.json recorded on the commit named there.  One case per (family, sky): nine renders of 32 x 32
pixels at 4 spp, the three integrators under the three drivers."""
import json

import numpy as np
import pytest

import test_shade_matrix as M


@pytest.mark.gpu
@pytest.mark.parametrize("family, sky", M.GROUPS)
def test_launch_matrix_renders_the_recorded_films(gpu_lib, mts, family, sky):
    golden = json.load(open(M.GOLDEN))["films"]
    films = M.render_group(mts, family, sky)
    assert len(films) == 9
    for cell, film in films.items():
        assert np.isfinite(film).all(), cell
        assert (film[..., :3] > 0).any(), cell
    differ = [cell for cell, film in films.items() if M.film_hash(film) != golden[cell]]
    assert not differ, "films differ from the recorded ones: %s" % ", ".join(differ)
