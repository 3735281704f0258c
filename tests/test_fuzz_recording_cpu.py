"""CPU tests of tools/fuzz_recording.py's generator and of tests/recording_ref.py (no GPU): the sweep that the suite runs
(test_gpu_parity.py::test_randomized_sweeps[fuzz_recording.py-N], seed 20261002) cannot quietly go blind.  Every test here runs
make_trial and the reference only, on exactly the suite's trials:

  * every path bucket of the plans and of the inputs is hit by at least three trials;
  * at most a quarter of the trials expect nothing but empty lists;
  * for each one-rule mutant of the reference below, the mutant's expected output differs from the true one in at least three
    trials -- so a kernel with that mistake fails the sweep;
  * recording_ref agrees with the restatements the existing tests carry, on three of their shapes.

If a count falls short, change the generator's probabilities in tools/fuzz_recording.py, not the assertion."""
import contextlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref
import recording_ref as ref
import timeline_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "fuzz_recording.py")
SEED, N = 20261002, 200                  # test_randomized_sweeps' seed and its trials for fuzz_recording.py
AT_LEAST = 3

_M = {}


def _tool():
    if "tool" not in _M:
        import lbaudiodetective_amd as lb
        if not os.path.exists(lb.LIB_PATH):                                  # (the plans are the library's own: conftest's lb does the same)
            lb.build()
        spec = importlib.util.spec_from_file_location("fuzz_recording", TOOL)
        _M["tool"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_M["tool"])
    return _M["tool"]


def _trials():
    """the suite's trials and their true expected values, made once"""
    if "trials" not in _M:
        tool = _tool()
        _M["trials"] = []
        for t in range(N):
            trial = tool.make_trial(tool.trial_rng(SEED, t))
            _M["trials"].append((trial, tool.expected(trial)))
    return _M["trials"]


def test_the_suite_runs_these_trials():
    """N and the seed are test_randomized_sweeps' own"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    assert '("fuzz_recording.py", %d)' % N in text and '"%d"' % SEED in text


def test_plan_only_needs_neither_torch_nor_a_gpu():
    """importing the tool imports no torch (the library's loader, which the plans go through, is the package's own business),
    and --plan-only runs with no device visible"""
    _tool()
    code = ("import importlib.util, sys\n"
            "spec = importlib.util.spec_from_file_location('fuzz_recording', %r)\n"
            "tool = importlib.util.module_from_spec(spec)\n"
            "spec.loader.exec_module(tool)\n"
            "assert 'torch' not in sys.modules\n"
            "assert tool.main(['3', '1', '--plan-only']) == 0\n" % TOOL)
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT,
                         env={**os.environ, "PYTHONPATH": ROOT, "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-1500:])
    assert "3 trials planned" in run.stdout and "occurrences:form_" in run.stdout


def test_a_trial_is_a_plain_dict_with_the_documented_keys():
    trial, want = _trials()[0]
    assert {"entries", "recordings", "L", "range", "thresholds", "capacities", "k", "index_base", "peaks", "scratch_limit", "grid_ceiling",
            "force_shared", "paths"} <= set(trial)
    assert len(want) == 14 and all(name + "_batch" in want for name in ("occurrences", "occurrences_peaks", "scores", "topk", "threshold",
                                                                         "timeline", "segments"))
    again = _tool().make_trial(_tool().trial_rng(SEED, 0))                    # a trial depends on (seed, trial) alone
    assert again["paths"] == trial["paths"] and all(np.array_equal(a, b) for a, b in zip(again["recordings"], trial["recordings"]))


def test_the_axes_stay_within_the_smallest_shapes():
    for trial, _want in _trials():
        lens = [len(e) for e in trial["entries"]]
        assert 1 <= len(lens) <= 200 and 1 <= min(lens) and max(lens) <= 1024
        assert 1 <= len(trial["recordings"]) <= 9 and len({len(r) for r in trial["recordings"]}) == 1
        assert 1 <= len(trial["recordings"][0]) <= 1100 and trial["L"] in _tool().L_VALUES
        assert trial["index_base"] + len(lens) <= 1 << 32 and trial["grid_ceiling"] in (0, 1, 2, 3)
        assert all(np.isfinite(t) and t > 0 for t in trial["thresholds"].values())


# ---- the path buckets --------------------------------------------------------------------------------------------------------------
FAMILY_BUCKETS = ("form_w", "form_s", "form_s_forced", "passes", "chunks", "tiles_1", "tiles_2_3", "tiles_4", "tiles_5_up")
BUCKETS = [f"{fam}:{b}" for fam in ("occurrences", "recording", "timeline") for b in FAMILY_BUCKETS] + [
    "entries_to_64", "entries_65_128", "entries_above_128", "case_a", "equal_length", "per_1", "odd_L", "range_below_L",
    "range_at_or_above_L", "grid_ceiling_1", "index_base", "capacity_cuts", "capacity_exact", "batch_empty_row", "k_above_positive"]


@pytest.mark.parametrize("bucket", BUCKETS)
def test_every_path_bucket_is_hit(bucket):
    hits = sum(bucket in trial["paths"] for trial, _want in _trials())
    print(bucket, hits)
    assert hits >= AT_LEAST


def test_the_buckets_are_what_the_plans_say():
    """a bucket is read off the library's own plan: the recorded limit gives the chunks and passes the bucket claims"""
    import lbaudiodetective_amd as lb
    for trial, _want in _trials():
        lens = [len(e) for e in trial["entries"]]
        R, per, n = len(trial["recordings"]), len(trial["recordings"][0]), len(lens)
        plan = lb.debug_occurrences_batch_plan(R, per, min(lens), max(lens), n, trial["scratch_limit"]["occurrences"])
        single = lb.debug_occurrences_batch_plan(1, per, min(lens), max(lens), n, trial["scratch_limit"]["occurrences"])
        assert ("occurrences:passes" in trial["paths"]) == (plan["recordings_per_pass"] < R)
        assert ("occurrences:chunks" in trial["paths"]) == (single["entries_per_chunk"] < n)
        assert ("occurrences:form_s" in trial["paths"]) == (plan["form"] == 0)
        if "occurrences:form_s_forced" in trial["paths"]:
            assert plan["form"] == 1 and trial["force_shared"]["occurrences"] and plan["tiles"] < 4


def test_most_trials_expect_something():
    empty = sum("all_empty" in trial["paths"] for trial, _want in _trials())
    assert 4 * empty <= N
    for trial, want in _trials():                                            # (the bucket is what the expected lists say)
        counts = [np.asarray(want[name][-1]).max() for name in want if name.split("_batch")[0] in
                  ("occurrences", "occurrences_peaks", "threshold", "segments")]
        assert ("all_empty" in trial["paths"]) == (not any(counts) and not want["timeline"][0].any() and not want["timeline_batch"][0].any())


# ---- the inputs discriminate: one-rule mutants of the reference -------------------------------------------------------------------------
def _peak_left_ge(q):
    m = np.ones(len(q), bool)
    m[1:] = q[1:] >= q[:-1]
    return m


def _peak_right_gt(q):
    m = np.ones(len(q), bool)
    m[:-1] = q[:-1] > q[1:]
    return m


def _best_offset_highest(q, best):
    at = np.flatnonzero(q == best)
    return int(at[-1]) if len(at) else 0


def _fold_highest_index(nq, profs, threshold, index_base=0):
    """timeline_ref.fold with equal scores going to the HIGHEST entry index"""
    keys, lengths, rank = np.zeros(nq, np.uint64), np.zeros(nq, np.uint32), np.zeros(nq, np.uint64)
    t = np.float32(threshold)
    for j, p in enumerate(profs):
        if p is None:
            continue
        ne, cells = p
        bits = cells.view(np.uint32).astype(np.uint64) << np.uint64(32)
        r = np.where(cells >= t, bits | np.uint64(j), np.uint64(0)).astype(np.uint64)
        better = r > rank[:len(r)]
        rank[:len(r)][better] = r[better]
        keys[:len(r)][better] = (bits | np.uint64(0xFFFFFFFF - (index_base + j)))[better]
        lengths[:len(r)][better] = ne
    return keys, lengths


def _greedy_higher_offset(keys, lengths):
    """timeline_ref.segments with equal keys visited from the HIGHER offset"""
    keys = np.asarray(keys).astype(np.uint64)
    taken, out = set(), []
    for o in sorted(range(len(keys)), key=lambda o: (-int(keys[o]), -o)):
        if keys[o] == 0:
            break
        span = range(o, o + int(lengths[o]))
        if any(x in taken for x in span):
            continue
        taken.update(span)
        out.append((o, 0xFFFFFFFF - (int(keys[o]) & 0xFFFFFFFF), np.uint32(int(keys[o]) >> 32).view(np.float32), int(lengths[o])))
    return sorted(out)


def _pair_words_range_rounded_down(bools, range_):
    """align_ref._pair_words with the range limit rounded DOWN to whole pairs"""
    b = np.asarray(bools, np.uint8)
    n, L = b.shape
    lim = min(range_ if range_ else L, L)
    pairs = (L + 1) // 2
    padded = np.zeros((n, 2 * pairs), np.uint8)
    padded[:, :L] = b
    first, second = padded[:, 0::2], padded[:, 1::2]

    def words(bits):
        full = np.zeros((n, 128), np.uint8)
        full[:, :pairs] = bits
        return np.packbits(full.reshape(n, 2, 64), axis=2, bitorder="little").view(np.uint64).reshape(n, 2)
    inside = np.zeros((1, 128), np.uint8)
    inside[0, :lim // 2] = 1
    P, N_ = words(first), words(second)
    rm = np.packbits(inside.reshape(1, 2, 64), axis=2, bitorder="little").view(np.uint64).reshape(1, 2)
    return P, N_, (P | N_) & rm


# name: (module, attribute, the mutated rule, the outputs it can change, the cells change too)
MUTANTS = {
    "peak rule: left compare >=": (ref, "peak_left", _peak_left_ge, ("occurrences_peaks",), False),
    "peak rule: right compare >": (ref, "peak_right", _peak_right_gt, ("occurrences_peaks",), False),
    "threshold: > instead of >=": (ref, "reaches", lambda q, t: q > np.float32(t), ("occurrences", "occurrences_peaks", "threshold"), False),
    "lag: the highest offset that reaches the maximum": (ref, "best_offset", _best_offset_highest, ("scores", "topk", "threshold"), False),
    "lag: the sign not flipped for longer entries": (ref, "lag_of", lambda offset, entry_long: -offset, ("scores", "occurrences"), False),
    "timeline: ties to the highest entry index": (ref, "fold", _fold_highest_index, ("timeline",), False),
    "segments: ties to the higher offset": (ref, "greedy", _greedy_higher_offset, ("segments",), False),
    "occurrences: the cut in (offset, entry) order": (ref, "occurrence_order", lambda entry, offset: np.lexsort((entry, offset)),
                                                      ("occurrences", "occurrences_peaks"), False),
    "top-K: equal scores by descending index": (ref, "topk_order", lambda sc: np.lexsort((-np.arange(len(sc)), -sc.astype(np.float64))),
                                                ("topk",), False),
    "range: the limit rounded down to whole pairs": (align_ref, "_pair_words", _pair_words_range_rounded_down, ("scores", "timeline"), True),
}


@contextlib.contextmanager
def _mutated(module, name, rule):
    true = getattr(module, name)
    setattr(module, name, rule)
    try:
        yield
    finally:
        setattr(module, name, true)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_inputs_tell_a_mutant_from_the_reference(mutant):
    module, name, rule, outputs, recompute = MUTANTS[mutant]
    tool = _tool()
    differing = 0
    for trial, want in _trials():
        if recompute:
            lim = min(trial["range"] or trial["L"], trial["L"])
            if lim % 2 == 0:                                                 # (whole pairs either way)
                continue
        with _mutated(module, name, rule):
            mine = trial
            if recompute:
                made = {}
                for rec in trial["recordings"]:
                    if rec.tobytes() not in made:
                        made[rec.tobytes()] = ref.cells(rec, trial["entries"], trial["range"])
                mine = {**trial, "cells": [made[rec.tobytes()] for rec in trial["recordings"]]}
            got = tool.expected(mine, only=outputs)
        differing += any(not tool.same_values(got[x], want[x]) for x in got)
        if differing >= AT_LEAST:
            break
    assert differing >= AT_LEAST, (mutant, differing)
    # and the rule is back: the reference gives the true values again
    trial, want = _trials()[0]
    assert all(tool.same_values(v, want[x]) for x, v in tool.expected(trial, only=outputs).items())


# ---- the reference agrees with what is there ------------------------------------------------------------------------------------------
def _expected_occurrences(profiles, t, peaks, index_base=0):
    """tests/test_gpu_occurrences.py's expected list, restated from its docstring: the cells >= float32(t) and, for peaks, (o == 0 or
    q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)), in (entry, offset) order; lag +o where the entry is the longer, else -o"""
    keys, lags = [], []
    for j, (q, entry_long) in enumerate(profiles):
        for o in range(len(q)):
            if not q[o] >= np.float32(t):
                continue
            if peaks and not ((o == 0 or q[o] > q[o - 1]) and (o == len(q) - 1 or q[o] >= q[o + 1])):
                continue
            keys.append((int(q[o:o + 1].view(np.uint32)[0]) << 32) | (0xFFFFFFFF - (index_base + j)))
            lags.append(o if entry_long else -o)
    return np.array(keys, np.uint64), np.array(lags, np.int32)


def _fixture(L, n_query, seed):
    """the existing tests' shape: 60 entries of 1..40 sub-fingerprints, one of 90 (longer than the query), one planted"""
    rng = np.random.default_rng(seed)
    tool = _tool()
    ent = [tool.rand_fp(rng, int(k), L, 0.02, 0.0) for k in rng.integers(1, 41, 60)]
    ent[5] = tool.rand_fp(rng, 90, L, 0.02, 0.0)
    q = tool.rand_fp(rng, n_query, L, 0.02, 0.0)
    q[20:20 + len(ent[9])] = ent[9]
    ent[5][20:20 + n_query] = q
    return q, ent


@pytest.mark.parametrize("L,range_", [(200, 63), (37, 0), (37, 20), (199, 0), (199, 64)])
def test_the_reference_agrees_with_the_restatements_that_exist(L, range_):
    q, ent = _fixture(L, 64, 1000 + L)
    cs = ref.cells(q, ent, range_)
    values = np.sort(np.concatenate([c for c, _ in cs]))
    distinct = np.unique(values)
    base = 12345
    assert cs[5][1] and len(cs[5][0]) == 90 - 64 + 1
    for t in (values[-1], distinct[-4], values[len(values) // 2], np.nextafter(values[-1], np.float32(np.inf))):
        for peaks in (False, True):
            keys, lags = _expected_occurrences(cs, t, peaks, base)
            for capacity in (len(keys) + 3, max(1, len(keys) // 2)):
                got = ref.occurrences(cs, t, peaks, capacity, base)
                m = min(len(keys), capacity)
                assert got[2] == len(keys) and np.array_equal(got[0][:m], keys[:m]) and np.array_equal(got[1][:m], lags[:m])
                assert not got[0][m:].any() and not got[1][m:].any() and len(got[0]) == capacity
        if t > 0:
            want = timeline_ref.timeline(q, ent, t, range_, base)
            got = ref.timeline(cs, len(q), t, base)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            spans = timeline_ref.segments(*want)
            st, sk, sl, count = ref.segments(*got, len(spans) + 2)
            assert count == len(spans) and st[:count].tolist() == [s[0] for s in spans] and sl[:count].tolist() == [s[3] for s in spans]
            assert np.array_equal(sk[:count], want[0][st[:count]]) and not sk[count:].any()
    sc, lags = ref.scores(cs)
    for j, e in enumerate(ent):
        best, lag = align_ref.align(q, e, range_)
        assert sc[j].view(np.uint32) == np.float32(best).view(np.uint32) and lags[j] == lag
    # top-K and threshold are the scores' selections
    keys, klags = ref.topk(cs, 7, base)
    order = sorted(range(len(ent)), key=lambda j: (-float(sc[j]), j))[:7]
    assert [0xFFFFFFFF - int(k & np.uint64(0xFFFFFFFF)) - base for k in keys] == order and klags.tolist() == [int(lags[j]) for j in order]
    t = np.sort(sc)[len(sc) // 2]
    keys, tlags, count = ref.threshold(cs, t, 10, base)
    at = [j for j in range(len(ent)) if sc[j] >= t]
    assert count == len(at) and [0xFFFFFFFF - int(k & np.uint64(0xFFFFFFFF)) - base for k in keys[:min(10, count)]] == at[:10]
    assert tlags[:min(10, count)].tolist() == [int(lags[j]) for j in at[:10]]
