"""tests/sched_cases.py reaches the edges it names, for every knob set the GPU schedule tests run — so that those tests cannot silently test
nothing when the grid formula (trt_handle::traceGrid) or the list of sizes changes."""
import numpy as np
import pytest

import sched_cases as SC

KNOB_SETS = SC.PERSISTENT_KNOBS + [g for g in SC.UNIFORM_GRIDS if g not in SC.PERSISTENT_KNOBS]
IDS = [SC.knob_id(e) for e in KNOB_SETS]


def test_grid_restatement_on_known_values():
    # the default handle: one block per 256 rays up to the 2048 blocks that fill the chip, then 1024 rays per block, in multiples of 8 blocks
    assert [SC.trace_grid(n) for n in (1, 2048, 2049, 300000, 524288, 524289, 1024 * 2049, 1 << 31)] == [8, 8, 16, 1176, 2048, 2048, 2056, 8192]
    assert SC.trace_grid(300000, fill_blocks=8) == 296           # test_gpu_records_written.py's overflow cases
    assert SC.trace_grid(10 ** 7, rays_per_wave=64) == 8192      # the other branch: one block per 256 rays, capped
    assert SC.trace_grid(10 ** 7, max_blocks=8) == 8
    assert SC.grid_knobs({"TRT_TRACE_MAXB": "3"}) == {"max_blocks": 8}  # trt_create: at least 8
    assert SC.parked_per_wave(300000, 2048).max() <= 128 < SC.parked_per_wave(300000, 8).min()


def test_the_small_grid_gives_the_sizes_the_design_names():
    sizes = [n for n, _ in SC.edge_sizes({"TRT_TRACE_MAXB": "8"})]
    assert all(SC.n_waves(n, {"TRT_TRACE_MAXB": "8"}) == 32 for n in sizes)
    assert set(sizes) >= {1, 31, 32, 33, 2047, 2048, 2049, 2080, 20000} and len(sizes) == 10


def test_knob_values_are_ones_trt_create_accepts():
    for env in SC.PERSISTENT_KNOBS:
        if "TRT_SCHED_W" in env:
            a, b = (int(x) for x in env["TRT_SCHED_W"].split(":"))
            assert 1 <= a <= 1023 and 1 <= b <= 1023
        if "TRT_REFILL_MIN" in env:
            assert 1 <= int(env["TRT_REFILL_MIN"]) <= 64
    assert len(SC.PERSISTENT_KNOBS) == 11 and len(SC.SWITCHES) == 4


@pytest.mark.parametrize("env", KNOB_SETS, ids=IDS)
def test_every_labelled_edge_occurs(env):
    sizes = SC.edge_sizes(env)
    by_label = {label: n for n, labels in sizes for label in labels}
    assert set(by_label) == set(SC.EDGE_LABELS), set(SC.EDGE_LABELS) ^ set(by_label)
    lengths = {n: SC.slice_lengths(n, env) for n, _ in sizes}

    # the slices of all waves partition [0, n), in wave order
    for n, _ in sizes:
        waves = SC.n_waves(n, env)
        assert waves % 32 == 0 and waves <= SC.MAX_TRACE_BLOCKS * SC.WAVES_PER_BLOCK
        first, end = SC.slice_bounds(n, waves)
        assert first[0] == 0 and end[-1] == n and (first <= end).all() and np.array_equal(first[1:], end[:-1])
        assert SC.wave_slices(n, waves)[0] == (0, int(end[0]))

    assert by_label["one-ray"] == 1 and lengths[1].tolist() == [1] + [0] * (SC.n_waves(1, env) - 1)
    for label, k in (("waves-1", -1), ("waves", 0), ("waves+1", 1)):
        n = by_label[label]
        assert n == SC.n_waves(n, env) + k
    assert (lengths[by_label["waves"]] == 1).all()                       # one ray per wave
    L = lengths[by_label["waves-1"]]
    assert (L[:-1] == 1).all() and L[-1] == 0                            # the last slice is empty: w0 >= n
    L = lengths[by_label["waves+1"]]
    assert L.max() == 2 and (L == 0).sum() >= len(L) // 2 - 1 and (L == 1).sum() == 1  # per = 2: half the slices are empty, one holds a single ray
    assert (lengths[by_label["per64"]] == 64).all()                      # every wave: exactly one refill batch
    L = lengths[by_label["per64-1"]]
    assert (L[:-1] == 64).all() and L[-1] == 63                          # a partial last slice
    assert by_label["per64+1"] == by_label["per64"] + 1 and lengths[by_label["per64+1"]].sum() == by_label["per64+1"]
    assert (lengths[by_label["per65"]] == 65).all()                      # every wave: a second refill that carries one ray
    L = lengths[by_label["one-ray-tail"]]
    filled = L[L > 0]
    assert filled[-1] == 1 and len(filled) > 1 and (filled[:-1] == filled[0]).all() and filled[0] > 2
    assert by_label["long"] == SC.LONG_N

    # and over the whole list: some wave with an empty slice, some wave with exactly one ray, every wave at 64, every wave at 65
    every = [L for L in lengths.values()]
    assert any((L == 0).any() for L in every) and any((L == 1).any() for L in every)
    assert any((L == 64).all() for L in every) and any((L == 65).all() for L in every)
