"""Frame phases without a device: the counts, the refusals and the sample-offset helper."""
import ctypes as C

import pytest

from phases_ref import PHASES_ALL, lengths_of

CONFIGS = ((2048, 64), (1024, 64), (512, 8), (4096, 64), (1024, 37))


def want_count(oracle, n_samples, window, stride, phases, phase):
    left = n_samples - phase * (128 // phases) * stride
    return oracle.subfingerprint_count(left, window, stride) if left >= window else 0


@pytest.mark.parametrize("window,stride", CONFIGS)
def test_count_at_phase_around_every_boundary(lb, oracle, window, stride):
    """L = window + (128 k + p h) stride - stride +- 1 sample, the same one stride later (where the reference's count, one window
    short of the windows that fit, changes), and everything down to an empty signal for the first boundary."""
    det = lb.Detective().configure(window=window, stride=stride)
    for phases in PHASES_ALL:
        h = 128 // phases
        lengths = {0, 1, window - 1, window, window + 1}
        for k in (0, 1, 2, 5):
            for p in range(phases):
                edge = window + (128 * k + p * h) * stride
                for at in (edge - stride, edge):
                    lengths.update(x for x in (at - 1, at, at + 1) if x >= 0)
        for n in sorted(lengths):
            got = [det.subfingerprint_count_at_phase(n, phases, p) for p in range(phases)]
            want = [want_count(oracle, n, window, stride, phases, p) for p in range(phases)]
            assert got == want, (phases, n)
            assert got[0] == det.subfingerprint_count(n)
            if got[0] >= 1:
                assert all(c in (got[0], got[0] - 1) for c in got) and got == sorted(got, reverse=True), (phases, n, got)


def test_batch_lengths_cover_what_they_are_for(oracle):
    """The clip lengths of the device tests hold a case with count_0 = 2 and one frame at every other phase, the same with the last
    phase's second frame just there and just not, and a case with one frame at phase 0 only."""
    for window, stride in ((2048, 64), (1024, 64), (512, 8)):
        for phases in PHASES_ALL:
            L = lengths_of(window, stride, phases)
            cnt = lambda n, p: want_count(oracle, n, window, stride, phases, p)   # noqa: E731
            assert [cnt(L["w256"], p) for p in range(phases)] == [2] + [1] * (phases - 1)
            assert [cnt(L["w256_last_gains"], p) for p in range(phases)] == [2] * phases
            assert [cnt(L["w256_last_gains_m1"], p) for p in range(phases)] == ([2] * (phases - 1) + [1] if phases > 1 else [1])
            assert [cnt(L["one_frame"], p) for p in range(phases)] == [1] + [0] * (phases - 1)
            assert cnt(L["one_frame_m1"], 0) == 0 and cnt(L["short"], 0) == 0


def test_refusals_without_a_device(lb):
    L = lb.lib()
    invalid = lb.constant("kLBAudioDetectiveArgumentInvalid")
    det = lb.Detective()
    n = 2048 + 64 * 1000
    for phases in (0, 3, 5, 6, 12, 48, 64, 128, 2**31):
        assert det.subfingerprint_count_at_phase(n, phases, 0) == 0
        # refused before anything is looked at: no device, no clips, no output
        assert L.LBAudioDetectiveFingerprintClipsDevicePhases(det._ref, None, 0, 0, n, phases, None, None) == invalid
    for phases in PHASES_ALL:
        assert det.subfingerprint_count_at_phase(n, phases, phases) == 0
        assert det.subfingerprint_count_at_phase(n, phases, 0) == det.subfingerprint_count(n) > 0
    assert L.LBAudioDetectiveGetSubfingerprintCountAtPhase(None, n, 4, 0) == 0
    assert L.LBAudioDetectiveFingerprintClipsDevicePhases(None, None, 0, 0, n, 4, None, None) == invalid
    # clips without a place for them, an output without a place
    assert L.LBAudioDetectiveFingerprintClipsDevicePhases(det._ref, None, 0, 1, n, 4, C.c_void_p(16), None) == invalid
    assert L.LBAudioDetectiveFingerprintClipsDevicePhases(det._ref, C.c_void_p(16), 0, 1, n, 4, None, None) == invalid
    assert L.LBAudioDetectiveFingerprintClipsDevicePhases(det._ref, C.c_void_p(16), 3, 1, n, 4, C.c_void_p(16), None) == invalid


def test_phase_sample_offset(lb):
    for stride in (1, 8, 64, 37):
        for phases in PHASES_ALL:
            h = 128 // phases
            assert [lb.phase_sample_offset(phases, p, stride) for p in range(phases)] == [p * h * stride for p in range(phases)]
            assert lb.phase_sample_offset(phases, 0, stride) == 0
            assert lb.phase_sample_offset(phases, phases - 1, stride) + h * stride == 128 * stride
    for phases, phase in ((0, 0), (3, 0), (64, 1), (4, 4), (4, -1), (1, 1)):
        with pytest.raises(ValueError):
            lb.phase_sample_offset(phases, phase, 64)
