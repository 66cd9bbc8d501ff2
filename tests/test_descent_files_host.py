"""CPU tier of the hand-made descent shapes (tests/descent_files.py): the byte surgery is the identity on a fixture's own
layers, the oracle loads every shape of every fixture, the shapes reach what they are for (census), and -- where the
compiled reference is present -- the reference's search of each file equals the oracle's.  The last one checks the
oracle's descent (oracle/cph_oracle.cpp: greedy_layer) on degrees, layer sizes, ties and depths no built index has,
before any kernel is compared with it."""
import numpy as np
import pytest

import descent_files as df
from golden_util import DATASETS
from oracle_lib import ref_available, ref_module

ALL_BITS = [(name, bits) for name, spec in DATASETS.items() for bits in spec["bits"]]
CASES = [(name, bits, shape) for name, bits in df.FIXTURES for shape in df.SHAPES_ALL]


@pytest.mark.parametrize("name,bits", ALL_BITS)
def test_own_layers_reproduce_the_file(name, bits):
    spec = DATASETS[name]
    data = df.fixture_bytes(name, bits)
    s = df.split_v2(data, spec, bits)
    layers = df.parse_upper(data, s["upper"][0])
    assert s["max_level"] == len(layers) > 0
    assert df.with_upper_layers(data, spec, bits, layers, s["entry"], s["max_level"]) == data
    assert df.with_equal_rows(data, spec, {}) == data


def test_equal_rows_touch_two_ranges_only():
    spec = DATASETS["g64"]
    data = df.fixture_bytes("g64", 4)
    out = df.with_equal_rows(data, spec, {5: 9})
    s = df.split_v2(out, spec, 4)
    X, D = df.raw_rows(out, spec, 4), spec["D"]
    assert np.array_equal(X[5], X[9]) and not np.array_equal(df.raw_rows(data, spec, 4)[5], X[9])
    diff = np.flatnonzero(np.frombuffer(out, np.uint8) != np.frombuffer(data, np.uint8))
    raw5, norm5 = s["raw"][0] + 5 * D * 4, s["norm_sq"][0] + 5 * 4
    assert len(diff) and all(raw5 <= i < raw5 + D * 4 or norm5 <= i < norm5 + 4 for i in diff)


@pytest.mark.parametrize("name,bits,shape", CASES)
def test_shape_loads_reaches_and_matches_the_reference(oracle, gold, tmp_path, name, bits, shape):
    made = df.make_shape(name, bits, shape, gold[f"Q/{name}"])
    spec = DATASETS[name]
    # the file says what the shape says
    s = df.split_v2(made["data"], spec, bits)
    assert df.parse_upper(made["data"], s["upper"][0]) == made["layers"]
    assert (s["entry"], s["max_level"]) == (made["entry"], made["max_level"])
    c = df.check_reach(name, shape, made)
    print(name, shape, "hops", dict(c["hops"]), "absent", dict(c["absent"]), "max moves", c["max_moves"],
          "ties", dict(c["ties"]), "equal best", c["equal_best"])
    p = tmp_path / "shape.idx"
    p.write_bytes(made["data"])
    oi = oracle.load(str(p))
    assert (oi.n, oi.max_level, oi.entry, oi.n_upper) == (spec["n"], made["max_level"], made["entry"], len(made["layers"]))
    ids, d, _ = oi.search_batch(made["Q"], 10)
    if ref_available():
        r = ref_module().CPIndex(spec["dim"], bits)
        r.load(str(p))
        rids, rd = r.search_batch(made["Q"], 10)
        assert np.array_equal(ids, rids) and d.tobytes() == rd.tobytes()
