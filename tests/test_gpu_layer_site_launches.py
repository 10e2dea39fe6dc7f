"""-m gpu: the launches of one training pass -- forward_loss(unit_grad=True) and its backward -- for every combination of the stages
behind the layer transform (root weight, layer norm, hidden dropout) and every route that runs them, against
tests/golden/layer_site_launches.json: the ORDERED names of the package's own kernels and the NUMBER of all other launches.  The
fixture was recorded by tests/golden/make_layer_site_launches.py on the commit before the layer routes were given one site policy
(kgwas_amd.model.LayerSite); the same recipe builds every case here.  An extra join_blocks copy, a lost in-place hand-over of the
next layer's blocks or a stage out of order shows as another list."""
import json

import pytest

from tests.golden import make_layer_site_launches as recipe

pytestmark = pytest.mark.gpu

with open(recipe.FIXTURE) as f:
    GOLDEN = json.load(f)


def test_the_fixture_covers_the_configurations():
    assert list(GOLDEN) == list(recipe.CONFIGS) and len(GOLDEN) == 15


@pytest.mark.parametrize('name', list(recipe.CONFIGS))
def test_launches_of_one_training_pass(tiny_kg, name):
    got, (dst, prefix), _ = recipe.record(tiny_kg, name)
    want = GOLDEN[name]
    print(f'{name}: {len(got["own"])} own launches (fixture {len(want["own"])}), {got["other"]} others (fixture {want["other"]}); '
          f'destination types per layer {dst}, proper-prefix (layer, type) pairs {prefix}')
    # the shapes at which a wrong block hand-over or a wrong slice of the root's input shows
    assert max(dst) >= 2, 'no layer with two destination types'
    assert prefix, 'no (layer, type) pair whose destination rows are a proper prefix of its input rows'
    assert got['own'] == want['own']
    assert got['other'] == want['other']
