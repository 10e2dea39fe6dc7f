"""-m gpu: the launches of every route that issues a weight / bias-gradient product, against
tests/golden/weight_grad_launches.json: the ORDERED names of the package's own kernels and the NUMBER of all other launches.  The
fixture was recorded by tests/golden/make_weight_grad_launches.py on the commit before those routes were given one job-record
builder (ops._tn_job), one eligibility rule (ops._tn_multi_ok) and one producer / optimiser hand-off (ops._hand_off); the same
recipe builds every case here.  A product that changed routes, a lost or an extra launch, or a workspace that became a fill shows
as another list."""
import json

import pytest

from tests.golden import make_weight_grad_launches as recipe

pytestmark = pytest.mark.gpu

with open(recipe.FIXTURE) as f:
    GOLDEN = json.load(f)

OP_CASES = [(name, with_sink) for name in recipe.OPS for with_sink in (False, True)]


def test_the_fixture_covers_the_cases():
    assert list(GOLDEN['steps']) == list(recipe.STEPS) and len(GOLDEN['steps']) == 8
    assert list(GOLDEN['ops']) == [recipe.op_key(*c) for c in OP_CASES] and len(GOLDEN['ops']) == 16


def _same(got, want, what):
    print(f'{what}: {len(got["own"])} own launches (fixture {len(want["own"])}), {got["other"]} others (fixture {want["other"]})')
    assert got['own'] == want['own']
    assert got['other'] == want['other']


@pytest.mark.parametrize('name', list(recipe.STEPS))
def test_launches_of_one_training_step(tiny_kg, monkeypatch, name):
    _same(recipe.record_step(tiny_kg, name, monkeypatch.setattr), GOLDEN['steps'][name], name)


@pytest.mark.parametrize('name,with_sink', OP_CASES)
def test_launches_of_one_op(monkeypatch, name, with_sink):
    got, _ = recipe.record_op(name, with_sink, monkeypatch.setattr)
    _same(got, GOLDEN['ops'][recipe.op_key(name, with_sink)], recipe.op_key(name, with_sink))
