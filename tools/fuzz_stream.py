#!/usr/bin/env python3
"""Randomized sweep of the host-buffer entry points against the oracle (not part of the test suite):
tools/fuzz_stream.py [trials] [seed].  Streaming (random chunkings, empty and tiny chunks included) must equal
ProcessPCM on the concatenation and the oracle; the host batch call must give the oracle's bits for float32, int16
and int32 clips; a stream bank fed random chunkings of several channels at once (device or host samples, any history and
pass size) must hand out, push by push, the oracle's rows of every channel and keep the last of them; a resampler bank (a random
rate pair of the tested set, random chunkings, device or host samples, float32 or int16, an occasional finish and reset) must emit,
push by push, the oracle converter's samples of every channel, bit for bit.
Round 2: 60 000 trials (seed 3), 0 mismatches, 452 s on one MI355X."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import lbaudiodetective_amd as lb
from oracle import oracle as O

trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
bad = 0
t0 = time.time()
for t in range(trials):
    kind = rng.integers(0, 4)
    if kind == 0:
        cfg = O.Config(44100, 1024)
    elif kind == 1:
        cfg = O.Config(5512, 2048)
    elif kind == 2:
        cfg = O.Config(48000, 4096)
    else:
        cfg = O.Config(float(rng.choice([8000, 11025, 16000, 22050])), int(2 ** rng.integers(5, 11)), int(rng.integers(8, 200)),
                       int(rng.integers(1, 65)), 1)
        cfg.subfp_len = int(rng.integers(1, min(256, 128 * cfg.bands) + 1))
    det = lb.Detective().configure(sample_rate=cfg.sample_rate, window=cfg.window, stride=cfg.stride, bands=cfg.bands,
                                   subfp_len=cfg.subfp_len)
    total = int(rng.integers(0, cfg.window + cfg.stride * 128 * 3 + 1000))
    pcm = O.synth_clip(int(rng.integers(0, 2**31)), 7, 44100, max(total, 1))[:total]
    leg = rng.integers(0, 4)
    if leg == 1:
        # ---- stream bank: several channels, one ragged push after the other ----
        import torch
        n_ch, hist = int(rng.integers(2, 6)), int(rng.integers(1, 7))
        sigs = [O.synth_clip(int(rng.integers(0, 2**31)), c, 44100, max(total, 1))[:int(rng.integers(0, total + 1))] for c in range(n_ch)]
        want = [O.fingerprint_pcm(x, cfg) if x.size >= cfg.window else np.zeros((0, cfg.subfp_len), np.uint8) for x in sigs]
        bank = lb.StreamBank(det, n_ch, hist, frames_per_pass=int(rng.choice([0, 1, 3])))
        at, ok = [0] * n_ch, True
        while ok and any(a < x.size for a, x in zip(at, sigs)):
            counts = [min(int(rng.choice([0, 1, int(rng.integers(1, 100)), int(rng.integers(100, 5000)), int(rng.integers(5000, 60000))])),
                          x.size - a) for a, x in zip(at, sigs)]
            chunks = [x[a:a + n] for a, x, n in zip(at, sigs, counts)]
            before = [O.subfingerprint_count(a, cfg.window, cfg.stride) for a in at]
            at = [a + n for a, n in zip(at, counts)]
            after = [O.subfingerprint_count(a, cfg.window, cfg.stride) for a in at]
            if rng.integers(0, 2) == 0:
                shift = int(rng.integers(0, 4))
                flat = torch.from_numpy(np.concatenate([np.zeros(shift, np.float32)] + chunks)).cuda()[shift:]
                new_counts, new = bank.push_device(flat, counts, new_out=True)
            else:
                new_counts, new = bank.push(chunks, new_out=True)
            rows = lb.unpack_packed(new.cpu().numpy(), cfg.subfp_len) if new.shape[0] else np.zeros((0, cfg.subfp_len), np.uint8)
            exp = np.concatenate([w[b:a] for w, b, a in zip(want, before, after)])
            ok = new_counts.tolist() == [a - b for a, b in zip(after, before)] and np.array_equal(rows, exp) and \
                bank.totals().tolist() == after
        for c in range(n_ch):
            if ok and want[c].shape[0]:
                ok = np.array_equal(bank.fingerprint(c).to_bools(), want[c][-hist:])
        bank.dispose()
        if not ok:
            bad += 1
            print("BANK MISMATCH", t, cfg.sample_rate, cfg.window, cfg.stride, cfg.bands, cfg.subfp_len, n_ch, hist, total, flush=True)
        continue
    if leg == 3:
        # ---- resampler bank: several channels, ragged pushes, finishes and resets ----
        import torch
        from math import gcd
        rate_in, rate_out, mode = [(44100, 5512, 0), (48000, 5512, 0), (8000, 44100, 0), (44100, 48000, 0), (44100, 5512, 1), (48000, 8000, 1)][int(rng.integers(0, 6))]
        p, q = rate_in // gcd(rate_in, rate_out), rate_out // gcd(rate_in, rate_out)
        m_hi = lb.debug_resampler_bank_plan(rate_in, rate_out, mode, [0], [0], [0])[3]
        n_ch, as_int = int(rng.integers(2, 6)), bool(rng.integers(0, 2))
        longest = 25000 if p > q else 5000
        raw = [np.round(O.synth_clip(int(rng.integers(0, 2**31)), c, rate_in, longest)[:int(rng.integers(0, longest + 1))] * 32767).astype(np.int16)
               for c in range(n_ch)]
        sigs = [x.astype(np.float32) * np.float32(1.0 / 32768.0) for x in raw]
        emitted = lambda L: 0 if L <= m_hi else -((L - m_hi) * q // -p)
        conv = lambda x: O.resample(x, rate_in, rate_out, mode)
        want = [conv(x) for x in sigs]
        bank = lb.ResamplerBank(rate_in, rate_out, n_ch, mode)
        start, at, ok = [0] * n_ch, [0] * n_ch, True
        while ok and any(a < x.size for a, x in zip(at, sigs)):
            event = int(rng.integers(0, 12))
            if event < 2:                                        # finish (0) or reset (1) a random set of channels
                chosen = [c for c in range(n_ch) if rng.integers(0, 2)]
                if event == 0:
                    whole = [conv(sigs[c][start[c]:at[c]]) for c in chosen]
                    new_counts, new = bank.finish(chosen)
                    exp = [w[emitted(at[c] - start[c]):] for c, w in zip(chosen, whole)]
                    ok = [int(new_counts[c]) for c in chosen] == [e.size for e in exp] and int(new_counts.sum()) == sum(e.size for e in exp) and \
                        np.array_equal(new.cpu().numpy().view(np.uint32), np.concatenate(exp + [np.zeros(0, np.float32)]).view(np.uint32))
                else:
                    bank.reset(chosen)
                for c in chosen:
                    start[c] = at[c]
                    want[c] = conv(sigs[c][at[c]:])
                continue
            counts = [min(int(rng.choice([0, 1, int(rng.integers(1, 100)), int(rng.integers(100, 3000)), int(rng.integers(3000, 12000))])),
                          x.size - a) for a, x in zip(at, sigs)]
            chunks = [(raw if as_int else sigs)[c][a:a + n] for c, (a, n) in enumerate(zip(at, counts))]
            before = [emitted(a - s) for a, s in zip(at, start)]
            at = [a + n for a, n in zip(at, counts)]
            after = [emitted(a - s) for a, s in zip(at, start)]
            if rng.integers(0, 2) == 0:
                shift = int(rng.integers(0, 4))
                flat = torch.from_numpy(np.concatenate([np.zeros(shift, chunks[0].dtype)] + chunks)).cuda()[shift:]
                new_counts, new = bank.push_device(flat, counts)
            else:
                new_counts, new = bank.push([ch.astype(np.int16 if as_int else np.float32) for ch in chunks])
            exp = np.concatenate([w[b:a] for w, b, a in zip(want, before, after)])
            totals = bank.totals()
            ok = new_counts.tolist() == [a - b for a, b in zip(after, before)] and totals[1].tolist() == after and \
                totals[0].tolist() == [a - s for a, s in zip(at, start)] and np.array_equal(new.cpu().numpy().view(np.uint32), exp.view(np.uint32))
        bank.dispose()
        if not ok:
            bad += 1
            print("RESAMPLER BANK MISMATCH", t, rate_in, rate_out, mode, n_ch, as_int, [x.size for x in sigs], flush=True)
        continue
    if leg == 0:
        # ---- streaming ----
        st = lb.Stream(det)
        at, emitted = 0, 0
        while at < total:
            c = int(rng.choice([0, 1, int(rng.integers(1, 100)), int(rng.integers(100, 5000)), int(rng.integers(5000, 60000))]))
            c = min(c, total - at)
            emitted += st.push(pcm[at:at + c])
            at += c
            if emitted != O.subfingerprint_count(at, cfg.window, cfg.stride):
                bad += 1
                print("STREAM COUNT MISMATCH", t, cfg.sample_rate, cfg.window, cfg.stride, cfg.bands, total, at, flush=True)
                break
        want = O.fingerprint_pcm(pcm, cfg) if total >= cfg.window else np.zeros((0, cfg.subfp_len), np.uint8)
        got = st.fingerprint().to_bools() if emitted else np.zeros((0, cfg.subfp_len), np.uint8)
        whole = det.process_pcm(pcm).to_bools() if want.shape[0] else got
        if got.shape[0] != want.shape[0] or (want.shape[0] and not (np.array_equal(got, want) and np.array_equal(whole, want))):
            bad += 1
            print("STREAM MISMATCH", t, cfg.sample_rate, cfg.window, cfg.stride, cfg.bands, cfg.subfp_len, total, flush=True)
        continue
    # ---- host batch, three sample formats ----
    n_clips = int(rng.integers(1, 6))
    spc = max(total, cfg.window + cfg.stride * 128)
    clips = O.synth_clips(int(rng.integers(0, 2**31)), 0, n_clips, 44100, spc)       # multiples of 1 / 32768
    want = O.fingerprint_batch(clips, cfg)
    got = det.fingerprint_clips(clips)
    i16 = np.round(clips * 32768).astype(np.int16)
    got16 = det.fingerprint_clips(i16)
    raw32 = rng.integers(-2**31, 2**31 - 1, clips.shape, dtype=np.int64).astype(np.int32)
    want32 = O.fingerprint_batch((raw32.astype(np.float64) / 2**31).astype(np.float32), cfg)
    got32 = det.fingerprint_clips(raw32)
    if not (np.array_equal(got, want) and np.array_equal(got16, want) and np.array_equal(got32, want32)):
        bad += 1
        print("HOST BATCH MISMATCH", t, cfg.sample_rate, cfg.window, cfg.stride, cfg.bands, cfg.subfp_len, n_clips, spc, flush=True)
print(f"{trials} trials, {bad} mismatches, {time.time() - t0:.1f} s")
sys.exit(1 if bad else 0)
