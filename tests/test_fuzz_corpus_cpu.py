"""CPU tests of tools/fuzz_corpus.py's generator and of tests/corpus_ref.py (no GPU): the sweep that the suite runs
(test_gpu_parity.py::test_randomized_sweeps[fuzz_corpus.py-N], seed 20261002) cannot quietly go blind.  Every test here runs
make_trial and the model only, on exactly the suite's trials:

  * every path bucket -- corpus kinds, mutations, the four steered states, read calls, knob value classes, which side slides,
    tile edges crossed from below and from above, capacities, key lists, chunks -- is hit by at least three trials;
  * at most a quarter of the threshold and join reads expect an empty list, at most a quarter of the removals remove nothing, at
    least half of the trials end with a non-empty corpus;
  * for each one-rule mutant of the model below, the mutant's expected words differ from the true ones in at least three trials
    -- so a kernel or a host path with that mistake fails the sweep;
  * the model agrees with the restatements the existing tests carry, and with the C oracle's corpus_best and scores (the only
    place the oracle is consulted).

If a count falls short, change the generator's probabilities in tools/fuzz_corpus.py, not the assertion."""
import contextlib
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import align_ref
import corpus_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "fuzz_corpus.py")
SEED, N = 20261002, 400                  # test_randomized_sweeps' seed and its trials for fuzz_corpus.py
AT_LEAST = 3

_M = {}


def _tool():
    if "tool" not in _M:
        spec = importlib.util.spec_from_file_location("fuzz_corpus", TOOL)
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


def _same(tool, a, b):
    """two results of expected(): every step's and every read's words"""
    return len(a) == len(b) and all(
        len(sa) == len(sb) and len(ra) == len(rb) and all(tool.same_values(x, y) for x, y in zip(list(sa) + list(ra), list(sb) + list(rb)))
        for (sa, ra), (sb, rb) in zip(a, b))


def test_the_suite_runs_these_trials():
    """N and the seed are test_randomized_sweeps' own"""
    text = open(os.path.join(ROOT, "tests", "test_gpu_parity.py")).read()
    assert '("fuzz_corpus.py", %d)' % N in text and '"%d"' % SEED in text


def test_plan_only_needs_neither_torch_nor_a_gpu():
    code = ("import importlib.util, sys\n"
            "spec = importlib.util.spec_from_file_location('fuzz_corpus', %r)\n"
            "tool = importlib.util.module_from_spec(spec)\n"
            "spec.loader.exec_module(tool)\n"
            "assert 'torch' not in sys.modules\n"
            "assert tool.main(['3', '1', '--plan-only']) == 0\n"
            "assert 'torch' not in sys.modules\n" % TOOL)
    run = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT,
                         env={**os.environ, "PYTHONPATH": ROOT, "HIP_VISIBLE_DEVICES": "", "ROCR_VISIBLE_DEVICES": ""})
    assert run.returncode == 0, (run.stdout[-1500:], run.stderr[-1500:])
    assert "3 trials planned" in run.stdout and "kind:" in run.stdout


def test_a_trial_is_a_plain_dict_that_depends_on_seed_and_trial_alone():
    tool = _tool()
    trial, want = _trials()[0]
    assert {"kind", "L", "n_sub", "entry_capacity", "record_capacity", "queries", "other", "stages", "paths", "variant", "pruning",
            "pruning_threshold", "grid_ceiling", "join_limit", "remove_limit", "range", "base_kind", "side_stream"} <= set(trial)
    assert len(want) == len(trial["stages"]) and all(len(r) == len(st["reads"]) for (_, r), st in zip(want, trial["stages"]))
    for t in (0, 7):
        a, b = tool.make_trial(tool.trial_rng(SEED, t)), tool.make_trial(tool.trial_rng(SEED, t))
        assert a["paths"] == b["paths"] and _same(tool, tool.expected(a), tool.expected(b))
        assert _same(tool, tool.expected(a), _trials()[t][1])
        assert all(np.array_equal(x, y) for x, y in zip(a["queries"], b["queries"]))


def test_the_axes_stay_within_the_smallest_shapes():
    tool = _tool()
    for trial, _want in _trials():
        steps = [s for st in trial["stages"] for s in st["steps"]]
        assert 3 <= len(trial["stages"]) - 1 <= 7 and all(4 <= len(st["reads"]) for st in trial["stages"])
        assert trial["L"] in (tool.L_UNIFORM if trial["kind"] == "uniform" else tool.L_RAGGED) and trial["grid_ceiling"] in (0, 1, 2, 3)
        model = ref.Model(trial["L"], trial["n_sub"], trial["range"])
        for st in steps:
            if st["op"] == "append":
                assert st is steps[0] or st is steps[1] or len(st["entries"]) <= 40     # (none: a loaded corpus without room)
                assert all((len(e) == trial["n_sub"]) if trial["kind"] == "uniform" else (1 <= len(e) <= 330) for e in st["entries"])
            tool.apply_step(model, trial, st)
            assert len(model) <= trial["entry_capacity"] and len(model) <= 2 * 4096 + 5 + 130
            assert trial["kind"] == "uniform" or model.total <= trial["record_capacity"]
        for st in trial["stages"]:
            for rd in st["reads"]:
                assert 0 <= rd["base"] <= 1 << 32 and ("t" not in rd or (np.isfinite(rd["t"]) and rd["t"] > 0))
                assert "k" not in rd or 1 <= rd["k"] <= 1024


def test_every_call_is_made_in_every_trial_whose_corpus_allows_it():
    """a trial that ends with a non-empty corpus makes every call; only the joins and the groups may be missing, the joins only
    outside their shapes (a uniform corpus of another length than 200, a ragged entry above the join's cap) and the groups also
    where no state of the trial is within the model's budget for n x n scores.  A trial that ends empty still makes the calls an
    empty corpus takes."""
    tool = _tool()
    full = 0
    joins = {"join_self", "join_other", "duplicate_groups"}
    for trial, _want in _trials():
        called = {rd["call"] for st in trial["stages"] for rd in st["reads"]}
        missing = set(tool.READS) - called
        assert set(tool.EMPTY_SAFE) <= called
        if trial["final_count"] > 0:
            assert missing <= joins, missing
            if trial["L"] == 200:
                assert missing <= {"duplicate_groups"}, missing
        full += not missing
    print(full, "of", N, "trials make every call")


# ---- the path buckets --------------------------------------------------------------------------------------------------------------
BUCKETS = (["kind:uniform", "kind:ragged", "wide", "small"]
           + ["mutation:" + m for m in ("append_packed", "append_fingerprint", "remove", "remove_keys", "remove_ids", "dedup", "save_load",
                                        "set_ids")]
           + ["state:" + s for s in ("count_returns", "through_empty", "ne_max_shrinks_and_grows", "ids_on_after_removal")]
           + ["read:" + r for r in ("query", "query_key_device", "query_batch", "query_packed_keys", "scores_device", "topk_host",
                                    "topk_keys", "topk_packed", "threshold_host", "threshold_keys", "threshold_packed", "align_keys",
                                    "match_profile", "join_self", "join_other", "duplicate_groups", "gather_keys", "gather", "gather_ids",
                                    "ids_from_keys", "keys_from_ids", "state")]
           + ["variant_%d" % v for v in range(5)] + ["pruning_on", "pruning_off"] + ["grid_ceiling_%d" % g for g in range(4)]
           + ["join_limit", "join_default", "remove_limit", "remove_default", "range_0", "range_below_L", "range_at_or_above_L", "odd_L",
              "index_base_0", "index_base_small", "index_base_top", "side_stream", "null_stream", "outputs_given", "outputs_allocated",
              "case_a", "equal_length", "case_b"]
           + ["edge_%d_from_%s" % (e, side) for e in (256, 1024, 2048, 4096) for side in ("below", "above")]
           + ["capacity_cuts", "capacity_exact", "k_above_positive", "keys_with_padding", "foreign_keys", "repeated_keys", "chunks:join",
              "chunks:remove", "dedup_redone_with_half_the_rows"])


@pytest.mark.parametrize("bucket", BUCKETS)
def test_every_path_bucket_is_hit(bucket):
    hits = sum(bucket in trial["paths"] for trial, _want in _trials())
    print(bucket, hits)
    assert hits >= AT_LEAST


def test_the_buckets_are_what_the_trials_say():
    """a bucket is read off the trial: the edges from the counts along the history, the empty state, the ids"""
    tool = _tool()
    for trial, _want in _trials():
        model, counts, on = ref.Model(trial["L"], trial["n_sub"], trial["range"]), [], []
        for st in [s for stage in trial["stages"] for s in stage["steps"]]:
            tool.apply_step(model, trial, st)
            counts.append(len(model))
            on.append(model.ids is not None)
        for edge in tool.EDGES:
            assert (f"edge_{edge}_from_below" in trial["paths"]) <= any(a < edge <= b for a, b in zip(counts, counts[1:]))
            assert (f"edge_{edge}_from_above" in trial["paths"]) <= any(a >= edge > b for a, b in zip(counts, counts[1:]))
        assert ("state:through_empty" in trial["paths"]) == any(a > 0 and b == 0 for a, b in zip(counts, counts[1:]))
        if "state:ids_on_after_removal" in trial["paths"]:
            first_on = on.index(True)
            assert any(b < a for a, b in zip(counts[:first_on], counts[1:first_on + 1]))
        assert trial["final_count"] == counts[-1]


def test_the_three_caps_on_the_generator():
    lists = [x for trial, _ in _trials() for x in trial["list_reads"]]
    removals = [x for trial, _ in _trials() for x in trial["removals"]]
    print(sum(lists), len(lists), sum(removals), len(removals), sum(trial["final_count"] > 0 for trial, _ in _trials()))
    assert 4 * sum(lists) <= len(lists)                                      # threshold and join reads that expect an empty list
    assert 4 * sum(removals) <= len(removals)                                # removals that remove nothing
    assert 2 * sum(trial["final_count"] > 0 for trial, _ in _trials()) >= N
    # (the flags are what the expected values say)
    checked = 0
    for trial, want in _trials():
        assert len(trial["list_reads"]) == len(_tool().list_reads(trial))
        for st, (_, reads) in zip(trial["stages"], want):
            for rd, r in zip(st["reads"], reads):
                if rd["call"] in ("threshold_host", "threshold_keys", "threshold_packed"):
                    count = r[3] if rd["call"] == "threshold_host" else r[1]
                    assert rd["empty"] == (int(np.max(count)) == 0)
                    checked += 1
                elif rd["call"] in ("join_self", "join_other"):
                    assert rd["empty"] == (int(r[-1][-1]) == 0)
                    checked += 1
    assert checked >= N


# ---- the inputs discriminate: one-rule mutants of the model -----------------------------------------------------------------------------
def _kept_but_the_last(n, indices):
    keep = np.ones(n, bool)
    idx = np.asarray(indices, np.int64)
    keep[idx] = False
    if len(idx):
        keep[idx.max()] = True
    return keep


MUTANTS = {
    "ties resolved highest index first": ("topk_order", lambda sc: np.lexsort((-np.arange(len(sc)), -sc.astype(np.float64)))),
    "> for >= at the threshold": ("reaches", lambda sc, t: sc > np.float32(t)),
    "a score of 0 admitted to top-K": ("admitted", lambda sc: sc >= 0),
    "threshold rows in descending order": ("threshold_order", lambda at: np.sort(at)[::-1]),
    "the lag sign flipped": ("lag_of", lambda offset, entry_long: np.where(entry_long, -offset, offset).astype(np.int32)),
    "the lag of the last offset that reaches the score": ("best_offset", lambda first, last: last),
    "a removal that leaves the last removed entry visible": ("kept_after", _kept_but_the_last),
    "ids that stay at their old positions after a removal": ("moved_ids", lambda ids, keep: list(ids)),
    "ids not cleared for appended entries": ("appended_id", lambda stale, position: stale.get(position, 0)),
    "skip_same_index ignored": ("pair_skipped", lambda row, entry, skip: False),
    "labels taken from one direction of the pairs only": ("edges_of", lambda pairs: [(a, b) for a, b in pairs if a < b]),
    "dedup keeping the last of a group": ("group_keeper", lambda members: members[-1]),
    "gather in ascending order, not list order": ("gather_rows", lambda named: np.sort(named)),
    "an index base applied to the wrong side of 0xFFFFFFFF -": (
        "low_word", lambda index, base: (np.uint64(ref.LOW) - np.asarray(index, np.int64).astype(np.uint64) + np.uint64(base)) & np.uint64(ref.LOW)),
}


@contextlib.contextmanager
def _mutated(name, rule):
    true = getattr(ref, name)
    setattr(ref, name, rule)
    try:
        yield
    finally:
        setattr(ref, name, true)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_inputs_tell_a_mutant_from_the_model(mutant):
    name, rule = MUTANTS[mutant]
    tool = _tool()
    differing = 0
    for trial, want in _trials():
        with _mutated(name, rule):
            try:
                got = tool.expected(trial)
            except (IndexError, ValueError, KeyError):                       # (the mutant's corpus no longer admits the trial's steps)
                got = None
        differing += got is None or not _same(tool, got, want)
        if differing >= AT_LEAST:
            break
    assert differing >= AT_LEAST, (mutant, differing)
    trial, want = _trials()[0]                                               # and the rule is back
    assert _same(tool, tool.expected(trial), want)


# ---- the model agrees with what is there ----------------------------------------------------------------------------------------------
def test_the_vectorised_scores_are_align_bit_for_bit():
    """score_block (one pass per entry length) against align_ref.align pair by pair, on a sample of every trial's own entries
    and queries -- wide trials, uniform ones and every range included"""
    pairs = 0
    for trial, _want in _trials()[:120]:
        entries = [e for st in trial["stages"] for s in st["steps"] if s["op"] == "append" for e in s["entries"]]
        sample = entries[:6] + entries[-6:] + trial["other"]
        for q in trial["queries"]:
            sc, first, last, longer = ref.score_block(q, sample, trial["range"])
            for j, e in enumerate(sample):
                best, lag = align_ref.align(q, e, trial["range"])
                assert ref.bits(best)[0] == ref.bits(sc[j])[0] and lag == (first[j] if longer[j] else -first[j]), (trial["L"], len(q), len(e))
                assert last[j] >= first[j] and bool(longer[j]) == (len(e) > len(q))
                pairs += 1
    assert pairs > 5000


def _fixture(L, seed, n=60):
    rng = np.random.default_rng(seed)
    tool = _tool()
    ent = [tool.rand_fp(rng, int(k), L, 0.02, 0.0) for k in rng.integers(1, 41, n)]
    ent[5] = tool.rand_fp(rng, 90, L, 0.02, 0.0)
    q = tool.rand_fp(rng, 30, L, 0.02, 0.0)
    q[3:3 + len(ent[9])][:len(q) - 3] = ent[9][:len(q) - 3]
    ent[5][20:50] = q
    ent[11], ent[n - 1] = ent[9].copy(), ent[9].copy()
    return q, ent


@pytest.mark.parametrize("L,range_", [(200, 0), (37, 20), (199, 64)])
def test_the_model_agrees_with_the_restatements_that_exist(L, range_):
    from test_gpu_groups import _union_find
    from test_gpu_remove import _expected
    from test_threshold_cpu import host_threshold_keys
    from test_topk_cpu import host_topk_keys
    q, ent = _fixture(L, 2000 + L)
    m = ref.Model(L, 0, range_)
    m.append(ent)
    sc, lags = m.scores("q", q)
    for j, e in enumerate(ent):
        best, lag = align_ref.align(q, e, range_)
        assert ref.bits(best)[0] == ref.bits(sc[j])[0] and lag == lags[j]
    base = 12345
    for k in (1, 7, len(ent) + 3):
        assert np.array_equal(m.topk(sc, lags, k, base)[0], host_topk_keys(sc, k, base).view(np.uint64))
    for t in (np.sort(sc)[len(sc) // 2], sc.max(), np.nextafter(sc.max(), np.float32(2))):
        for capacity in (1, 10, len(ent)):
            keys, _, count, _, _ = m.threshold(sc, lags, t, capacity, base)
            want_keys, want_count = host_threshold_keys(sc, t, capacity, base)
            assert count == want_count and np.array_equal(keys, want_keys.view(np.uint64))
    assert m.top1(sc, base)[0] == host_topk_keys(sc, 1, base).view(np.uint64)[0]
    # the components of the self-join's pairs
    values = np.unique(np.concatenate([np.delete(m.scores(qid, e)[0], r) for r, qid, e in m.self_rows(0, len(m))]))
    for t in (values[-1], values[-3], values[len(values) // 2]):
        pairs = m.join(m.self_rows(0, len(m)), t, 1, True)[3]
        lab, groups = m.labels(t)
        want = _union_find(len(m), pairs)
        assert np.array_equal(lab, want) and groups == len(set(want.tolist()))
    # the removal's map, and what is left
    for indices in ([0, 3, 3, 59], list(range(0, 60, 2)), [], list(range(60))):
        mm = ref.Model(L, 0, range_)
        mm.append(ent)
        mm.set_ids(0, list(range(100, 160)))
        keep, new, removed = _expected(60, indices)
        got_removed, got_new = mm.remove(indices)
        assert got_removed == removed and np.array_equal(got_new, new)
        assert all(np.array_equal(a, b) for a, b in zip(mm.bools(), [e for e, k in zip(ent, keep) if k]))
        assert mm.entry_ids().tolist() == [100 + i for i in range(60) if keep[i]]


@pytest.mark.parametrize("L,range_", [(200, 0), (64, 33), (199, 120)])
def test_the_model_agrees_with_the_oracle(oracle, L, range_):
    """corpus_best and the per-entry scores of the C oracle, on a ragged and on a uniform corpus: the only place it is consulted"""
    q, ent = _fixture(L, 3000 + L, n=40)
    rg = range_ if range_ else L
    for query in (q, ent[9], ent[5]):
        m = ref.Model(L, 0, range_)
        m.append(ent)
        sc, _ = m.scores("q", query)
        bi, bs, want = oracle.corpus_best_ragged(query, ent, rg, want_scores=True)
        assert np.array_equal(ref.bits(sc), ref.bits(want))
        _, idx, s = m.top1(sc)
        assert idx == bi and ref.bits(s)[0] == ref.bits(bs)[0]
    tool = _tool()
    rng = np.random.default_rng(L)
    uni = np.stack([tool.rand_fp(rng, 5, L, 0.02, 0.05) for _ in range(50)])
    uni[30] = uni[4]
    m = ref.Model(L, 5, range_)
    m.append(list(uni))
    for query in (uni[4], tool._noisy(rng, uni[17], 0.05), np.zeros((5, L), np.uint8)):
        sc, _ = m.scores(("u", query.tobytes()), query)
        _, idx, s = m.top1(sc)
        bi, bs = oracle.corpus_best(query, uni, rg)
        assert idx == bi and ref.bits(s)[0] == ref.bits(bs)[0]
        if L == 200:
            want = oracle.corpus_scores_packed(oracle.pack_bools(query), oracle.pack_bools(uni), L, rg)
            assert np.array_equal(ref.bits(sc), ref.bits(want))
