"""The packed weight layouts (csrc/amtx_pack_layouts.h) through the op-level HOST packers of the product library, no GPU: the SHA-256
of every packed buffer against tests/golden/pack_layouts.json, which tools/gen_golden_pack_layouts.py recorded on the commit before the
layouts became one definition each for the host and device packers (cases and inputs: that file's docstring)."""
import importlib.util
import json
import os

import pytest

from amt_tools_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def recorded():
    spec = importlib.util.spec_from_file_location('gen_golden_pack_layouts', os.path.join(ROOT, 'tools', 'gen_golden_pack_layouts.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, 'tests', 'golden', 'pack_layouts.json')) as f:
        want = json.load(f)
    assert want['seed'] == gen.SEED
    return gen.record(_lib.lib(), _lib.ptr), want


def test_every_packed_buffer_is_the_recorded_one(recorded):
    got, want = recorded
    assert got['skipped'] == want['skipped']
    # 2 c_out + 6 channel pairs, x 2 planes x 2 scales; 6 Linear shapes, 4 hidden sizes and the hidden-128 entry point, x 2 planes
    assert len(want['hashes']) + 2 * len(want['skipped']) == (2 + 6) * 4 + (6 + 4 + 1) * 2
    assert list(got['hashes']) == list(want['hashes'])
    wrong = [k for k in want['hashes'] if got['hashes'][k] != want['hashes'][k]]
    assert not wrong, wrong


def test_hidden_128_packs_alike_through_both_entry_points(recorded):
    got, _ = recorded
    for planes in (1, 2):
        assert got['hashes'][f'bilstm 128 planes {planes}'] == got['hashes'][f'bilstm_h 128 planes {planes}']
