"""GPU parity of the pruned stage 1 (k_rows_pruned.hip) where every workgroup both prefetches a span and claims frames, on the
plan 44.1 kHz / 1024 / 64: the claim is a global atomic issued right behind the span prefetch, and the LDS reads that follow
the prefetch inside an iteration do not wait for it (tests/test_isa_rows_waits.py pins the compiled loop).

264 clips of 44 100 samples are 1 320 frames, the smallest batch in which every persistent workgroup of a 256-CU device takes
one frame statically and then claims: 165 frames per XCD, 64 taken by the 64 workgroups of the XCD, 101 claimed from its counter.
9 clips are 45 frames: six per XCD and three on the last one, whose other workgroups leave at once through the ticket.  Every
result is compared with the CPU oracle bit for bit, under both band-sum forms, twice through one Detective (the second launch
relies on the counters the first one left at zero), and on int16 input (the converting span loader, 40 clips)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATE, WINDOW, STRIDE = 44100, 1024, 64
SAMPLES = 44100
CLIPS = 264
SEED = 0x4C424144


@pytest.fixture(scope="module")
def reference(lb, gpu, oracle):
    """The clips on the device and the oracle's bits of each, computed once and left unchanged."""
    cfg = oracle.Config(RATE, WINDOW)
    clips = lb.synth_clips_device(SEED, 0, CLIPS, RATE, SAMPLES)
    gpu.cuda.synchronize()
    host = clips.cpu().numpy()
    assert np.array_equal(host, oracle.synth_clips(SEED, 0, CLIPS, RATE, SAMPLES)), "device PCM generator differs from the oracle's"
    want = oracle.fingerprint_batch(host, cfg)
    want.setflags(write=False)
    host.setflags(write=False)
    return cfg, clips, host, want


def _det(lb, form):
    det = lb.Detective().configure(sample_rate=RATE, window=WINDOW, stride=STRIDE)
    det.set_band_sum_form(form)
    assert det.band_sum_form() == form
    return det


def _twice(lb, gpu, det, clips, length):
    """Two calls through one Detective: (bits of the first, packed bytes of both)."""
    first = det.fingerprint_clips_device(clips)
    second = det.fingerprint_clips_device(clips)
    gpu.cuda.synchronize()
    a, b = first.cpu().numpy(), second.cpu().numpy()
    return lb.unpack_packed(a, length).reshape(a.shape[0], a.shape[1], length), a, b


def _check(lb, gpu, clips, want, length, what):
    packed = {}
    for form in (1, 2):
        bits, a, b = _twice(lb, gpu, _det(lb, form), clips, length)
        assert np.array_equal(a, b), f"{what}: the second call differs from the first (form {form})"
        assert bits.shape == want.shape, (bits.shape, want.shape)
        wrong = np.flatnonzero((bits != want).reshape(bits.shape[0], -1).any(axis=1))
        assert wrong.size == 0, f"{what}: clips {wrong[:8].tolist()} differ from the oracle (form {form})"
        packed[form] = a
    assert np.array_equal(packed[1], packed[2]), f"{what}: the two band-sum forms differ"


def test_every_workgroup_prefetches_and_claims(lb, gpu, reference):
    cfg, clips, _, want = reference
    frames = CLIPS * want.shape[1]
    assert want.shape[1] == 5 and frames == 1320
    # two persistent workgroups per CU, an eighth of them and of the frames per XCD: every workgroup has a frame of its own and
    # there are frames left to claim for each of them
    wg_per_xcd = (2 * gpu.cuda.get_device_properties(0).multi_processor_count + 7) // 8
    assert frames // 8 >= 2 * wg_per_xcd, (frames, wg_per_xcd)
    _check(lb, gpu, clips, want, cfg.subfp_len, "264 clips")


def test_short_ranges_and_workgroups_that_leave_at_once(lb, gpu, reference):
    cfg, clips, _, want = reference
    assert 9 * want.shape[1] == 45
    _check(lb, gpu, clips[:9].contiguous(), want[:9], cfg.subfp_len, "9 clips")


def test_int16_input(lb, gpu, oracle, reference):
    cfg, _, host, _ = reference
    ints = np.clip(np.rint(host[:40].astype(np.float64) * 8000.0), -32768, 32767).astype(np.int16)
    assert np.abs(ints).max() > 100, "the quantised clips are not silent"
    want = oracle.fingerprint_batch((ints.astype(np.float64) / 32768.0).astype(np.float32), cfg)
    _check(lb, gpu, gpu.from_numpy(ints).cuda(), want, cfg.subfp_len, "40 int16 clips")
