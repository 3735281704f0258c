"""Frame phases on the device: every output word against the oracle on the shifted signal.

The law: the sub-fingerprints of phase p of P of a signal x[0, L) are oracle.fingerprint_pcm(x[p * h * stride : L]) with
h = 128 / P, packed with oracle.pack_bools.  A frame depends on its own windows only, so the oracle runs once per (clip,
offset) on the longest signal of a configuration and a shorter signal's expectation is its first count rows -- the count being
oracle.subfingerprint_count(L - offset)."""
import numpy as np
import pytest

from phases_ref import PHASES_ALL, lengths_of

pytestmark = pytest.mark.gpu

POISON = 0xA5
N_CLIPS = 3

# name -> (rate, window, stride, bands, subfp_len, stage-2 family the batch call reaches, compact rows between the stages)
CONFIGS = {
    "default": (5512, 2048, 64, 32, 200, "select32", False),
    "headline": (44100, 1024, 64, 32, 200, "select32_sparse", True),
    # 48 kHz / 4096 has no compact plan (only 44.1 kHz / 1024 has one in the batch call: the sparse form without the 44.1 kHz mask
    # is reached through LBAudioDetectiveCompactFramesToSubfingerprintsDevice alone); it is here for its stage 1, as are the next two
    "stream48k": (48000, 4096, 64, 32, 200, "select32", False),
    "full32k": (32000, 1024, 64, 32, 200, "select32", False),
    "pruned48k": (48000, 1024, 64, 32, 200, "select32", False),
    "bands16": (5512, 2048, 64, 16, 200, "select32", False),
    "bands64": (5512, 2048, 64, 64, 200, "select32", False),
    "generic": (5512, 512, 8, 24, 200, "generic", False),
}


class Case:
    """One configuration's three master clips (int16, so that sample formats 0 and 1 carry the same signal) and the oracle's
    sub-fingerprints from every offset a phase can have, computed when first asked for and kept."""

    def __init__(self, name, oracle):
        self.rate, self.window, self.stride, self.bands, self.subfp_len, self.stage2, self.compact = CONFIGS[name]
        self.cfg = oracle.Config(self.rate, self.window, self.stride, self.bands, self.subfp_len)
        self.oracle = oracle
        self.l_max = self.window + (256 + 128 + 128) * self.stride
        rng = np.random.default_rng(0x50484153 + sum(name.encode()))
        self.pcm16 = rng.integers(-20000, 20000, size=(N_CLIPS, self.l_max), dtype=np.int16)
        # a quiet stretch and a loud one, so that not every frame looks alike
        self.pcm16[1, 3000:5000] //= 64
        self.pcm16[2, : self.l_max // 2] //= 4
        self.pcm32 = (self.pcm16.astype(np.float32) / np.float32(32768.0)).astype(np.float32)
        self._words = {}

    def words(self, clip, offset):
        """[frames, 8] uint32: the oracle on the master clip from sample `offset` on."""
        key = (clip, offset)
        if key not in self._words:
            bools = self.oracle.fingerprint_pcm(self.pcm32[clip, offset:], self.cfg)
            self._words[key] = self.oracle.pack_bools(bools).view(np.uint32).reshape(-1, 8)
        return self._words[key]

    def expected(self, n_samples, phases):
        """[clips, phases, count_0, 8] uint32 and [phases] counts for clips cut to n_samples."""
        h = 128 // phases
        count0 = self.oracle.subfingerprint_count(n_samples, self.window, self.stride) if n_samples >= self.window else 0
        want = np.zeros((N_CLIPS, phases, count0, 8), np.uint32)
        counts = []
        for p in range(phases):
            off = p * h * self.stride
            left = n_samples - off
            cnt = self.oracle.subfingerprint_count(left, self.window, self.stride) if left >= self.window else 0
            counts.append(cnt)
            for c in range(N_CLIPS):
                want[c, p, :cnt] = self.words(c, off)[:cnt]
        return want, counts


_cases = {}


@pytest.fixture
def case(request, oracle):
    name = request.param
    if name not in _cases:
        _cases[name] = Case(name, oracle)
    return _cases[name]


def detective(lb, case):
    return lb.Detective().configure(sample_rate=case.rate, window=case.window, stride=case.stride, bands=case.bands,
                                    subfp_len=case.subfp_len)


def run_batch(torch, det, case, n_samples, phases, fmt):
    src = case.pcm16 if fmt == 1 else case.pcm32
    clips = torch.from_numpy(np.ascontiguousarray(src[:, :n_samples])).cuda()
    count0 = det.subfingerprint_count(n_samples)
    out = torch.full((N_CLIPS, phases, count0, 32), POISON, dtype=torch.uint8, device="cuda")
    det.fingerprint_clips_device_phases(clips, phases, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(N_CLIPS, phases, count0, 8)


def check_batch(torch, lb, case, phases, fmts=(0, 1)):
    det = detective(lb, case)
    for tag, n_samples in lengths_of(case.window, case.stride, phases).items():
        want, counts = case.expected(n_samples, phases)
        for p in range(phases):
            assert det.subfingerprint_count_at_phase(n_samples, phases, p) == counts[p], (tag, p)
        assert counts[0] == want.shape[2] and all(c in (counts[0], max(counts[0], 1) - 1) for c in counts), (tag, counts)
        for fmt in fmts:
            got = run_batch(torch, det, case, n_samples, phases, fmt)
            assert got.shape == want.shape, (tag, fmt)
            bad = np.argwhere((got != want).any(axis=-1))
            assert bad.size == 0, f"{tag} ({n_samples} samples), format {fmt}, P {phases}: (clip, phase, frame) {bad[:8].tolist()} differ"
    return det


@pytest.mark.parametrize("phases", PHASES_ALL)
@pytest.mark.parametrize("case", ["default", "headline"], indirect=True)
def test_batch_phases(gpu, lb, case, phases):
    det = check_batch(gpu, lb, case, phases)
    ch = det.stage1_choice(0, N_CLIPS, case.window + 256 * case.stride)
    assert ch.stage2 == case.stage2 and ch.compact == case.compact, ch


STAGE1 = {"stream48k": "stream", "full32k": "full", "pruned48k": "pruned", "bands16": "full", "bands64": "generic", "generic": "full"}


@pytest.mark.parametrize("case", ["stream48k", "full32k", "pruned48k", "bands16", "bands64", "generic"], indirect=True)
def test_batch_phases_other_kernels(gpu, lb, case, request):
    det = detective(lb, case)
    ch = det.stage1_choice(0, N_CLIPS, case.window + 256 * case.stride)
    assert ch.family == STAGE1[request.node.callspec.params["case"]], ch
    assert ch.stage2 == case.stage2 and ch.compact == case.compact, ch
    check_batch(gpu, lb, case, 4)


@pytest.mark.parametrize("case", ["default", "headline"], indirect=True)
def test_batch_phases_in_two_chunks(gpu, lb, case):
    """The scratch limit holds two clips' rows (count_0 frames and the tail frame each): three clips take two chunks."""
    torch = gpu
    det = detective(lb, case)
    phases = 8
    n_samples = lengths_of(case.window, case.stride, phases)["w256_last_gains_m1"]
    want, _ = case.expected(n_samples, phases)
    det.set_scratch_limit(2 * (want.shape[2] + 1) * 128 * case.bands * 4)
    for fmt in (0, 1):
        got = run_batch(torch, det, case, n_samples, phases, fmt)
        assert np.array_equal(got, want), fmt


@pytest.mark.parametrize("case", ["default", "headline", "generic"], indirect=True)
def test_one_phase_is_the_batch_call(gpu, lb, case):
    torch = gpu
    det = detective(lb, case)
    for n_samples in (case.window + 256 * case.stride + 17, case.l_max):
        clips = torch.from_numpy(np.ascontiguousarray(case.pcm32[:, :n_samples])).cuda()
        plain = det.fingerprint_clips_device(clips)
        phased = det.fingerprint_clips_device_phases(clips, 1)
        torch.cuda.synchronize()
        assert phased.shape == (N_CLIPS, 1, plain.shape[1], 8)
        assert np.array_equal(phased.cpu().numpy().view(np.uint8).reshape(plain.shape), plain.cpu().numpy())


@pytest.mark.parametrize("case", ["default"], indirect=True)
def test_batch_refusals(gpu, lb, case):
    torch = gpu
    det = detective(lb, case)
    clips = torch.from_numpy(np.ascontiguousarray(case.pcm32[:, : case.window + 256 * case.stride])).cuda()
    for phases in (0, 3, 5, 64, 128):
        out = torch.full((N_CLIPS, max(phases, 1), 2, 32), POISON, dtype=torch.uint8, device="cuda")
        with pytest.raises(lb.LBAudioDetectiveError):
            det.fingerprint_clips_device_phases(clips, phases, out=out)
        torch.cuda.synchronize()
        assert bool((out == POISON).all())
    # a clip shorter than a window: success, nothing written
    short = torch.from_numpy(np.ascontiguousarray(case.pcm32[:, : case.window - 1])).cuda()
    got = det.fingerprint_clips_device_phases(short, 4)
    assert got.shape == (N_CLIPS, 4, 0, 8)


# ---- the phased stream bank --------------------------------------------------------------------------------------------------
BANK_CHANNELS, BANK_HISTORY = 3, 4


class BankModel:
    """Three channels of seeded noise and, per virtual channel, what the law says it holds: oracle.fingerprint_pcm on the channel's
    samples since its last reset without the phase's offset -- run once per (channel, first sample, offset) on everything the test
    will ever push (a frame depends on its own windows only) and cut to the count of the samples pushed so far."""

    def __init__(self, name, oracle):
        self.rate, self.window, self.stride, self.bands, self.subfp_len = CONFIGS[name][:5]
        self.cfg = oracle.Config(self.rate, self.window, self.stride, self.bands, self.subfp_len)
        self.oracle = oracle
        self.hop = 128 * self.stride
        rng = np.random.default_rng(0x42414E4B + sum(name.encode()))
        self.sig = (rng.standard_normal((BANK_CHANNELS, self.window + 13 * self.hop)) * 0.25).astype(np.float32)
        self._words = {}

    def words(self, channel, start, offset):
        key = (channel, start, offset)
        if key not in self._words:
            bools = self.oracle.fingerprint_pcm(self.sig[channel, start + offset:], self.cfg)
            self._words[key] = self.oracle.pack_bools(bools).view(np.uint32).reshape(-1, 8)
        return self._words[key]

    def count(self, n_samples, offset):
        left = n_samples - offset
        return self.oracle.subfingerprint_count(left, self.window, self.stride) if left >= self.window else 0

    def windows(self, n_samples):
        return (n_samples - self.window) // self.stride + 1 if n_samples >= self.window else 0


_bank_models = {}


def bank_model(name, oracle):
    if name not in _bank_models:
        _bank_models[name] = BankModel(name, oracle)
    return _bank_models[name]


class BankRun:
    """A phased bank and the model's view of it; push() pushes and checks everything a push can be asked for."""

    def __init__(self, lb, torch, model, phases, frames_per_pass=0, history=BANK_HISTORY):
        self.lb, self.torch, self.m, self.phases, self.history = lb, torch, model, phases, history
        self.h = 128 // phases
        self.det = lb.Detective().configure(sample_rate=model.rate, window=model.window, stride=model.stride, bands=model.bands,
                                            subfp_len=model.subfp_len)
        self.bank = lb.StreamBank(self.det, BANK_CHANNELS, history, frames_per_pass=frames_per_pass, phases=phases)
        assert self.bank.phases == phases and self.bank.virtual_channels == BANK_CHANNELS * phases
        assert lb.lib().LBAudioDetectiveStreamBankGetPhases(self.bank._ref) == phases
        self.start = [0] * BANK_CHANNELS          # first sample of the channel's present life
        self.at = [0] * BANK_CHANNELS             # samples of the signal consumed
        self.allowed = 0                          # the windows the cost condition allows so far
        self.lives = []                           # (channel, samples) of the lives a reset ended

    def offset(self, p):
        return self.lb.phase_sample_offset(self.phases, p, self.m.stride)

    def want_counts(self):
        return [self.m.count(self.at[c] - self.start[c], self.offset(p)) for c in range(BANK_CHANNELS) for p in range(self.phases)]

    def want_words(self, c, p, lo, hi):
        return self.m.words(c, self.start[c], self.offset(p))[lo:hi]

    def push(self, counts, host=False, history=True):
        torch, bank = self.torch, self.bank
        before = self.want_counts()
        chunks = [self.m.sig[c, self.at[c]:self.at[c] + counts[c]] for c in range(BANK_CHANNELS)]
        assert all(len(chunks[c]) == counts[c] for c in range(BANK_CHANNELS)), "the model's signals are too short for this test"
        for c in range(BANK_CHANNELS):
            self.at[c] += counts[c]
        after = self.want_counts()
        fresh = [a - b for a, b in zip(after, before)]
        if host:
            new_counts, new = bank.push(chunks, new_out=True)
        else:
            flat = np.concatenate(chunks) if sum(counts) else np.zeros(0, np.float32)
            new_counts, new = bank.push_device(torch.from_numpy(flat).cuda(), counts, new_out=True)
        torch.cuda.synchronize()
        assert new_counts.tolist() == fresh, (counts, new_counts.tolist(), fresh)
        assert bank.totals().tolist() == after
        want_new = [self.want_words(c, p, before[c * self.phases + p], after[c * self.phases + p])
                    for c in range(BANK_CHANNELS) for p in range(self.phases)]
        want_new = np.concatenate(want_new) if want_new else np.zeros((0, 8), np.uint32)
        got_new = new.cpu().numpy().view(np.uint32).reshape(-1, 8)
        assert got_new.shape == want_new.shape and np.array_equal(got_new, want_new), \
            f"new sub-fingerprints differ at {np.argwhere((got_new != want_new).any(axis=-1))[:8].ravel().tolist()}"
        for c in range(BANK_CHANNELS):          # a push that completed a frame on a channel earns the channel 128 windows
            if any(fresh[c * self.phases:(c + 1) * self.phases]):
                self.allowed += 128
        if history:
            self.check_history()
        return fresh

    def check_history(self):
        """WindowDevice and CopyFingerprint of every virtual channel"""
        torch, bank = self.torch, self.bank
        counts = self.want_counts()
        for n in sorted({min(c, self.history) for c in counts if c}):
            listed = [v for v, c in enumerate(counts) if c >= n]
            got = bank.window_device(listed, n)
            torch.cuda.synchronize()
            got = got.cpu().numpy().view(np.uint32).reshape(len(listed), n, 8)
            for i, v in enumerate(listed):
                c, p = divmod(v, self.phases)
                assert np.array_equal(got[i], self.want_words(c, p, counts[v] - n, counts[v])), (v, n)
        for v, cnt in enumerate(counts):
            c, p = divmod(v, self.phases)
            fp = bank.fingerprint(v)
            keep = min(cnt, self.history)
            assert fp.number_of_subfingerprints == keep, (v, cnt)
            if keep:
                got = self.m.oracle.pack_bools(fp.to_bools()).view(np.uint32).reshape(-1, 8)
                assert np.array_equal(got, self.want_words(c, p, cnt - keep, cnt)), v

    def reset(self, channel):
        self.bank.reset([channel])
        self.lives.append((channel, self.at[channel] - self.start[channel]))
        self.start[channel] = self.at[channel]

    def check_work(self):
        """the cost condition: at most the windows of every life's samples plus 128 per (channel, push) that completed a frame"""
        windows, frames = self.bank.work()
        lives = self.lives + [(c, self.at[c] - self.start[c]) for c in range(BANK_CHANNELS)]
        have = sum(self.m.windows(n) for _, n in lives)
        assert windows <= have + self.allowed, (windows, have, self.allowed)
        assert windows >= have - 3 * len(lives)                 # ... and nothing but the last windows of a life is left out
        return windows, frames


def bank_pushes(model):
    """The issue's patterns on three channels; `None` resets channel 1.  Chunks of 1, stride - 1 and 128 stride + 1 samples first."""
    W, S, hop = model.window, model.stride, model.hop
    return [
        [1, S - 1, 0],                            # a channel without samples; no frame
        [S - 1, 1, 0],                            # no frame
        [hop + 1, W + hop + 39 * S, 0],           # channel 1 has window + (128 + 40) strides: a frame at the phases up to 40 rows in
        [3 * hop, 1, W + 1],                      # three frames' worth in one push
        [5 * hop + 17, 6 * hop, 5 * hop + S],     # more frames than the history holds
        None,
        [hop, W + 2 * hop, 1],                    # channel 1 from its new first sample
        [S - 1, hop + 1, hop],
    ]


@pytest.mark.parametrize("phases,frames_per_pass", [(1, 0), (4, 0), (4, 2), (32, 0)])
@pytest.mark.parametrize("name", ["default", "headline"])
def test_phased_bank(gpu, lb, oracle, name, phases, frames_per_pass):
    model = bank_model(name, oracle)
    run = BankRun(lb, gpu, model, phases, frames_per_pass)
    some_only = False
    for i, counts in enumerate(bank_pushes(model)):
        if counts is None:
            others = [c for v, c in enumerate(run.want_counts()) if v // phases != 1]
            run.reset(1)
            assert [c for v, c in enumerate(run.bank.totals().tolist()) if v // phases != 1] == others
            assert run.bank.totals().tolist() == run.want_counts() and run.bank.pending()[1] == 0
            run.check_history()
            continue
        fresh = run.push(counts, host=i % 3 == 2)
        if i < 2:
            assert not any(fresh)
        ch1 = fresh[phases:2 * phases]
        some_only = some_only or (any(ch1) and not all(ch1))
        run.check_work()
    assert some_only == (phases > 1), "no push completed frames at some phases of a channel only"
    assert max(run.want_counts()) > BANK_HISTORY
    run.check_work()


@pytest.mark.parametrize("phases", [1, 4, 32])
@pytest.mark.parametrize("name", ["default", "headline"])
def test_phased_bank_in_one_push(gpu, lb, oracle, name, phases):
    """The samples the chunked test gives every channel before its reset, in ONE push."""
    model = bank_model(name, oracle)
    run = BankRun(lb, gpu, model, phases)
    pushes = bank_pushes(model)
    totals = [sum(p[c] for p in pushes[:pushes.index(None)]) for c in range(BANK_CHANNELS)]
    run.push(totals)
    windows, _ = run.check_work()
    assert windows <= sum(model.windows(n) for n in totals)          # (one push: the 128-window allowance is not needed)


@pytest.mark.parametrize("name", ["default", "headline"])
def test_phased_bank_work_does_not_depend_on_the_phases(gpu, lb, oracle, name):
    """GetWork of the same samples -- the chunked pushes with their reset, and one push -- at P = 1, 4 and 32 and at two pass
    sizes, all inside this test: the windows transformed are the same everywhere, the frames selected the same at one P whatever
    the passes, and P times the windows' worth of frames is what the phases cost."""
    model = bank_model(name, oracle)
    pushes = bank_pushes(model)
    chunked, one = {}, {}
    for phases, frames_per_pass in ((1, 0), (4, 0), (4, 2), (32, 0)):
        run = BankRun(lb, gpu, model, phases, frames_per_pass)
        for i, counts in enumerate(pushes):
            if counts is None:
                run.reset(1)
            else:
                run.push(counts, host=i % 3 == 2, history=False)
        chunked[(phases, frames_per_pass)] = run.check_work()
        if frames_per_pass == 0:
            run = BankRun(lb, gpu, model, phases)
            run.push([sum(p[c] for p in pushes[:pushes.index(None)]) for c in range(BANK_CHANNELS)], history=False)
            one[phases] = run.check_work()
    assert len({w for w, _ in chunked.values()}) == 1 and len({w for w, _ in one.values()}) == 1, (chunked, one)
    assert chunked[(4, 0)] == chunked[(4, 2)], chunked
    assert chunked[(1, 0)][1] < chunked[(4, 0)][1] < chunked[(32, 0)][1] and one[1][1] < one[4][1] < one[32][1], (chunked, one)


def test_phased_bank_refusals(gpu, lb, oracle):
    torch = gpu
    model = bank_model("headline", oracle)
    invalid = lb.constant("kLBAudioDetectiveArgumentInvalid")
    det = lb.Detective().configure(sample_rate=model.rate, window=model.window, stride=model.stride)
    L = lb.lib()
    for phases in (0, 3, 64):
        assert not L.LBAudioDetectiveStreamBankNewPhased(det._ref, 3, 4, 0, phases)
    assert not L.LBAudioDetectiveStreamBankNewPhased(None, 3, 4, 0, 4) and not L.LBAudioDetectiveStreamBankNewPhased(det._ref, 0, 4, 0, 4)
    assert not L.LBAudioDetectiveStreamBankNewPhased(det._ref, 3, 0, 0, 4)
    assert L.LBAudioDetectiveStreamBankGetPhases(None) == 0
    plain = lb.StreamBank(det, 3, 4)
    assert plain.phases == 1 and L.LBAudioDetectiveStreamBankGetPhases(plain._ref) == 1
    with pytest.raises(lb.LBAudioDetectiveError):
        plain.work()
    run = BankRun(lb, torch, model, 4)
    run.push([model.window + 2 * model.hop + 100 * model.stride, model.window + model.hop, 0])
    nv = run.bank.virtual_channels
    totals, pending = run.bank.totals(), run.bank.pending()
    out = torch.full((2, BANK_HISTORY + 1, 32), POISON, dtype=torch.uint8, device="cuda")
    # a virtual channel out of range, a window longer than the history, than a listed channel's total
    for channels, n in (([0, nv], 1), ([0], BANK_HISTORY + 1), ([0, run.bank.virtual(1, 3)], 2), ([run.bank.virtual(2, 0)], 1)):
        with pytest.raises(lb.LBAudioDetectiveError) as err:
            run.bank.window_device(channels, n, out=out)
        assert err.value.status == invalid
    assert not L.LBAudioDetectiveStreamBankCopyFingerprint(run.bank._ref, nv)
    with pytest.raises(lb.LBAudioDetectiveError):
        run.bank.reset([BANK_CHANNELS])                       # reset takes REAL channels
    # room for fewer sub-fingerprints than the push completes: refused, nothing changes
    counts = [model.hop, model.hop, model.window + model.hop]
    chunks = [model.sig[c, run.at[c]:run.at[c] + counts[c]] for c in range(BANK_CHANNELS)]
    small = torch.full((2, 32), POISON, dtype=torch.uint8, device="cuda")
    with pytest.raises(lb.LBAudioDetectiveError) as err:
        run.bank.push_device(torch.from_numpy(np.concatenate(chunks)).cuda(), counts, new_out=small)
    assert err.value.status == invalid
    torch.cuda.synchronize()
    assert bool((out == POISON).all()) and bool((small == POISON).all())
    assert np.array_equal(run.bank.totals(), totals) and np.array_equal(run.bank.pending(), pending)
    run.check_history()
    run.push(counts)                                          # the same push with room


# ---- a planted airing, end to end ------------------------------------------------------------------------------------------
def test_planted_airing_is_found_at_its_phase(gpu, lb, oracle):
    """A four-frame clip goes to air 3 x 128 + 3 x 16 rows into a channel: off the channel's frame grid, on the grid of phase 3 of
    8.  The phase-3 virtual channel reports the entry with score 1.0 at the frame it starts in, and lag and phase give back the
    sample; phase 0 -- all the parent commit can be asked for -- reports nothing at that threshold."""
    torch = gpu
    rate, window, stride, bands, length = CONFIGS["headline"][:5]
    cfg = oracle.Config(rate, window, stride, bands, length)
    phases, hop = 8, 128 * stride
    h = 128 // phases
    frames_in, planted_phase, clip_frames = 3, 3, 4
    rng = np.random.default_rng(0x41495249)
    clip = (rng.standard_normal(window + clip_frames * hop) * 0.25).astype(np.float32)
    entry = oracle.fingerprint_pcm(clip, cfg)
    assert entry.shape[0] == clip_frames
    # (L - window) / stride = 128 x 9 + 120: the same count at all eight phases
    channel = (rng.standard_normal(window + (128 * 9 + 120) * stride) * 0.25).astype(np.float32)
    at = frames_in * hop + planted_phase * h * stride
    assert at == frames_in * hop + lb.phase_sample_offset(phases, planted_phase, stride)
    channel[at:at + clip.size] = clip
    # the oracle's view, before anything runs on the device: phase 3 holds the entry, phase 0 never reaches 1.0 against it
    by_phase = [oracle.fingerprint_pcm(channel[lb.phase_sample_offset(phases, p, stride):], cfg) for p in range(phases)]
    count = by_phase[0].shape[0]
    assert all(f.shape[0] == count for f in by_phase) and count == 9
    assert np.array_equal(by_phase[planted_phase][frames_in:frames_in + clip_frames], entry)
    best0 = max(oracle.compare_fp(by_phase[0][j:j + clip_frames], entry, length) for j in range(count - clip_frames + 1))
    assert best0 < 1.0, best0

    det = lb.Detective().configure(sample_rate=rate, window=window, stride=stride, bands=bands, subfp_len=length)
    corpus = lb.Corpus.ragged(length, 16, 128)
    others = np.random.default_rng(0x434F5250)
    for i in range(8):
        corpus.append_fingerprint(lb.Fingerprint.from_bools(others.integers(0, 2, size=(2 + i % 5, length), dtype=np.uint8)))
    corpus.append_fingerprint(lb.Fingerprint.from_bools(entry))
    planted_index = 8

    bank = lb.StreamBank(det, 1, count, phases=phases)
    new_counts, _ = bank.push([channel])
    assert new_counts.tolist() == [count] * phases
    virtual = [bank.virtual(0, p) for p in range(phases)]
    keys, lags, counts = bank.occurrences(corpus, virtual, count, 1.0, 16, peaks=True)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy().tolist()
    assert counts == [1 if p == planted_phase else 0 for p in range(phases)], counts
    idx, score, lag = lb.decode_occurrence_keys(keys[planted_phase], lags[planted_phase], counts[planted_phase])
    assert idx.tolist() == [planted_index] and score.tolist() == [1.0]
    # the occurrences' lag convention: lag = -o places the entry at sub-fingerprint o of the window, here of the whole phase
    assert int(lag[0]) == -frames_in
    assert lb.phase_sample_offset(phases, planted_phase, stride) + -int(lag[0]) * 128 * stride == at
