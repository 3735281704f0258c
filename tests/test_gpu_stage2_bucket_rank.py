"""Stage 2's candidate list is laid out by histogram bucket (the 11 leading bits of |v|) and a candidate is ranked inside its
bucket's segment; a frame with a segment longer than 64 keys, or whose threshold the bisection or the plateau path refines,
keeps the all-pairs ranking (k_haar_select32.hip).  Every case here is a handful of frames built for ONE bucket occupancy,
mostly by an inverse Haar transform in float64 of chosen coefficients; the oracle's coefficients of the float32 frame must
show that occupancy before the device's bits are compared with the oracle's, bit for bit, through the compile-time sparse
instance (44.1 kHz / 1024 compact frames), the run-time-position sparse instance (another plan of 30 .. 60 kHz) and the
general forms of 16, 32 and 64 columns, with keep = 1, 100 and 128.

The CPU test at the end reads the compiled kernels' resource usage: no scratch in any instance, and the sparse instances
still fit ten workgroups per CU (at most 64 VGPRs, no more LDS than before the bucket ranking)."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, KCAND, SEG_CAP = 128, 128, 64
TOP_BUCKET = (127 + 6) << 3            # |v| in [64, 72)


# ---- building frames -----------------------------------------------------------------------------------------------------
def inv_haar_1d(a):
    """Inverse of the oracle's haar_1d along the last axis, float64."""
    a = np.array(a, np.float64)
    n, cnt = a.shape[-1], 1
    while cnt < n:
        s, d = a[..., :cnt].copy(), a[..., cnt:2 * cnt].copy()
        a[..., 0:2 * cnt:2] = (s + d) / math.sqrt(2.0)
        a[..., 1:2 * cnt:2] = (s - d) / math.sqrt(2.0)
        cnt *= 2
    return a * math.sqrt(n)


def inv_haar_2d(c):
    return inv_haar_1d(inv_haar_1d(np.asarray(c, np.float64).T).T)


def free_columns(live):
    """Ordered positions of a transformed row whose basis function lies inside the live bands: a frame made of them alone
    has exact zeros in every other band."""
    n, out, size = len(live), [], 2
    while size <= n:
        out += [n // size + blk for blk in range(n // size) if live[blk * size:(blk + 1) * size].all()]
        size *= 2
    return sorted(out + ([0] if live.all() else []))


def centre(bucket, u=0.5):
    """A magnitude inside histogram bucket `bucket`, a fraction u of the way through it."""
    return math.ldexp(1.0 + ((bucket & 7) + u) / 8.0, (bucket >> 3) - 127)


def own_buckets(first, n):
    return [centre(first - i) for i in range(n)]


def in_one_bucket(bucket, n):
    return [centre(bucket, u) for u in np.linspace(0.9, 0.1, n)]


def occupancy(haar, keep):
    """The kernel's search on the oracle's coefficients: which ranking the frame takes and its candidates per bucket."""
    bits = np.ascontiguousarray(haar, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)
    above = np.cumsum(np.bincount(bits >> 20, minlength=2048)[::-1])[::-1]
    ok = np.nonzero(above[1:] >= keep)[0]                    # bucket 0 is never the histogram's answer
    if ok.size == 0:
        lo, hi, cnt, refined = 0, 1 << 20, bits.size, True
    else:
        b = int(ok[-1]) + 1
        lo, hi, cnt = b << 20, (b + 1) << 20, int(above[b])
        refined = cnt > KCAND
    while cnt > KCAND and hi - lo > 1:
        mid = lo + ((hi - lo) >> 1)
        c = int((bits >= mid).sum())
        if c >= keep:
            lo, cnt = mid, c
        else:
            hi = mid
    if cnt > KCAND:
        order = np.lexsort((np.arange(bits.size), -bits.astype(np.int64)))[:keep]
        cand, path = bits[order], "plateau"
    else:
        cand = bits[bits >= lo]
        path = "bisection" if refined else None
    seg = np.bincount(cand >> 20, minlength=2048)
    seg = seg[seg > 0]
    if path is None:
        path = "segments" if seg.max() <= SEG_CAP else "crowded"
    return {"path": path, "lo": lo, "nc": int(cand.size), "seg": seg, "cand": cand, "nonzero": int((bits != 0).sum())}


def build_cases(oracle, live, keep, seed):
    """name -> (frame [128, bands] float32, check(occupancy, haar))"""
    bands = len(live)
    rng = np.random.default_rng(seed)
    cols = free_columns(live)
    assert len(cols) >= 3, cols
    slots = [(r, c) for r in range(ROWS) for c in cols]
    live_bands = np.nonzero(live)[0]
    cases = {}

    def from_coefficients(name, magnitudes, check):
        at = rng.permutation(len(slots))[:len(magnitudes)]
        c = np.zeros((ROWS, bands))
        for m, s in zip(magnitudes, at):
            c[slots[s]] = m * rng.choice((-1.0, 1.0))
        frame = inv_haar_2d(c).astype(np.float32)
        assert not frame[:, ~live].any(), name
        cases[name] = (frame, check)

    def check_own(o, haar):
        assert o["path"] == "segments" and o["nc"] == keep and o["seg"].max() == 1, (o["path"], o["nc"], o["seg"])
    from_coefficients("own_bucket_each", own_buckets(TOP_BUCKET, keep + 10), check_own)

    def check_one(o, haar):
        assert o["path"] == "crowded" and len(o["seg"]) == 1 and o["nc"] == max(keep, 120), (o["path"], o["nc"], o["seg"])
    from_coefficients("all_in_one_bucket", in_one_bucket(TOP_BUCKET, max(keep, 120)), check_one)

    n_above = min(20, keep - 1)
    for extra, path in ((0, "segments"), (1, "crowded")):
        n_in = SEG_CAP + extra
        n_below = max(0, keep - n_above - n_in)
        mags = own_buckets(TOP_BUCKET, n_above) + in_one_bucket(TOP_BUCKET - n_above, n_in) + own_buckets(TOP_BUCKET - n_above - 1, n_below + 10)

        def check_cap(o, haar, n_in=n_in, path=path, n_below=n_below):
            assert o["path"] == path and o["seg"].max() == n_in and o["nc"] == n_above + n_in + n_below, (o["path"], o["nc"], o["seg"])
        from_coefficients(f"longest_segment_{n_in}", mags, check_cap)

    def check_bisect(o, haar):
        assert o["path"] == "bisection" and keep <= o["nc"] <= KCAND and (o["lo"] & 0xFFFFF) != 0, (o["path"], o["nc"], hex(o["lo"]))
    from_coefficients("bisection_inside_a_bucket", own_buckets(TOP_BUCKET, min(10, keep - 1)) + in_one_bucket(TOP_BUCKET - 12, 140), check_bisect)

    typical = ((np.abs(rng.standard_normal((ROWS, bands))) * 40.0).astype(np.float32) * live).astype(np.float32)
    cases["typical"] = (typical, lambda o, haar: None)

    # Rows 64 .. 127 = minus rows 0 .. 63 exactly: the coefficient at row position p of the first half of a level comes with
    # its negative at the position half a level further down, so every bucket holds one magnitude twice, with both signs
    # and two flat indices (a frame whose halves mirror each other transforms into coefficients that do, operation by operation).
    halves = [(p, p + cnt // 2) for cnt in (2, 4, 8, 16, 32, 64) for p in range(cnt, cnt + cnt // 2)]
    twins = [(halves[i], c) for i in rng.permutation(len(halves)) for c in cols][:keep // 2 + 6]
    c = np.zeros((ROWS, bands))
    for m, ((p, q), col) in zip(own_buckets(TOP_BUCKET, len(twins)), twins):
        c[p, col] = m * rng.choice((-1.0, 1.0))
        c[q, col] = -c[p, col]
    mirrored = inv_haar_2d(c).astype(np.float32)
    assert np.array_equal(mirrored[64:], -mirrored[:64]) and not mirrored[:, ~live].any()

    def check_ties(o, haar):
        v = haar.reshape(-1)
        order = np.lexsort((np.arange(v.size), -(v.view(np.uint32) & np.uint32(0x7FFFFFFF)).astype(np.int64)))[:2 * ((keep + 1) // 2)]
        top = v[order]
        assert o["path"] == "segments" and o["nc"] == len(top) and (o["seg"] == 2).all(), (o["path"], o["nc"], o["seg"])
        assert (top[0::2] == -top[1::2]).all() and (order[0::2] < order[1::2]).all()
    cases["equal_magnitudes_both_signs"] = (mirrored, check_ties)

    # (-1)^row (-1)^band on the pairs of live bands: 64 equal coefficients per pair, and three times that in rows 0 and 1
    pairs = [b for b in range(0, bands, 2) if live[b] and live[b + 1]]
    assert len(pairs) >= 3, pairs
    plateau = np.zeros((ROWS, bands), np.float32)
    for b in pairs:
        plateau[:, b] = np.where(np.arange(ROWS) % 2 == 0, 1.5, -1.5)
        plateau[:, b + 1] = -plateau[:, b]
    if keep > len(pairs):
        plateau[:2] *= 3.0                                   # (keys above the plateau, where they do not fill `keep` by themselves)

    def check_plateau(o, haar):
        assert o["path"] == "plateau" and o["nonzero"] == 64 * len(pairs), (o["path"], o["nonzero"])
    cases["plateau"] = (plateau, check_plateau)

    def check_silence(o, haar):
        assert o["path"] == "plateau" and o["lo"] == 0 and o["nonzero"] == 0
    cases["digital_silence"] = (np.zeros((ROWS, bands), np.float32), check_silence)

    few = np.zeros((ROWS, bands), np.float32)
    few[5, live_bands[0]] = 3.0
    if bands <= 32:                                          # (one value leaves 8 (log2 bands + 1) non-zero coefficients)
        few[77, live_bands[-1]] = -2.0

    def check_few(o, haar):
        assert o["nonzero"] >= 1 and (keep < 100 or (o["nonzero"] < keep and o["path"] == "plateau" and o["lo"] == 0)), (o["nonzero"], o["path"])
    cases["fewer_non_zero_than_kept"] = (few, check_few)

    tiny = np.zeros((ROWS, bands), np.float32)
    tiny[9, live_bands[-1]] = np.float32(2.0 ** -117)        # coefficients from 2^-124 down: normal and denormal ones

    def check_denormal(o, haar):
        denormal = (o["cand"] != 0) & (o["cand"] < 0x00800000)
        assert keep < 100 or (o["nonzero"] < keep and denormal.sum() >= 4 and (o["cand"] >= 0x00800000).sum() >= 4), (o["nonzero"], int(denormal.sum()))
    cases["denormal_candidates"] = (tiny, check_denormal)

    nan = typical.copy()
    nan[77, live_bands[-1]] = np.nan

    def check_nan(o, haar):
        n = int(np.isnan(haar).sum())
        assert 1 <= n < 100 and not np.isinf(haar).any(), n
    cases["one_nan"] = (nan, check_nan)

    inf = typical.copy()
    inf[10, live_bands[-1]] = np.inf
    inf[90, live_bands[0]] = -np.inf

    def check_inf(o, haar):
        assert np.isinf(haar).sum() >= 16
    cases["infinities"] = (inf, check_inf)
    return cases


def reference(oracle, cases, keep, subfp_len):
    """Oracle coefficients and bits of every case, after the case's own occupancy check."""
    want = {}
    for name, (frame, check) in cases.items():
        with np.errstate(invalid="ignore", over="ignore"):
            haar = oracle.haar_2d(frame)
            check(occupancy(haar, keep), haar)
        want[name] = (haar, oracle.extract(haar, subfp_len)[:subfp_len])
    return want


FORMS = ["sparse_44k", "sparse_runtime", "general_16", "general_32", "general_64"]


def form_setup(lb, oracle, form, subfp_len):
    """(detective, live bands, compact)"""
    def live_of(rate, window):
        _, lo, hi = oracle.band_table(rate, window)
        return np.asarray(lo) < np.asarray(hi)
    if form == "sparse_44k":
        det = lb.Detective().configure(sample_rate=44100, window=1024, subfp_len=subfp_len)
        assert lb.compact_layout(det) == (13, 21)
        return det, live_of(44100, 1024), True
    if form == "sparse_runtime":
        live44 = live_of(44100, 1024)
        for window in (2048, 512, 1024):
            for rate in range(30000, 60001, 250):
                live = live_of(rate, window)
                if np.array_equal(live[16:], live44[16:]) and live[:16].any():
                    continue                                 # (the compile-time instance's right half with a live band on the left)
                det = lb.Detective().configure(sample_rate=rate, window=window, subfp_len=subfp_len)
                lay = lb.compact_layout(det)
                if lay is not None and lay[1] <= 21 and len(free_columns(live)) >= 3:
                    return det, live, True
        raise AssertionError("no second plan with a compact layout")
    bands = int(form.split("_")[1])
    return lb.Detective().configure(sample_rate=44100, window=1024, bands=bands, subfp_len=subfp_len), np.ones(bands, bool), False


@pytest.mark.gpu
@pytest.mark.parametrize("subfp_len", [1, 200, 255])
@pytest.mark.parametrize("form", FORMS)
def test_bucket_ranking_bit_exact(lb, gpu, oracle, form, subfp_len):
    keep = (subfp_len + 1) // 2
    det, live, compact = form_setup(lb, oracle, form, subfp_len)
    cases = build_cases(oracle, live, keep, seed=1000 + FORMS.index(form))
    want = reference(oracle, cases, keep, subfp_len)
    frames = np.stack([f for f, _ in cases.values()])
    assert frames.shape[0] <= 64
    packed, haar = lb.frames_to_subfingerprints_device(det, gpu.from_numpy(frames).cuda(), want_haar=True, compact=compact)
    gpu.cuda.synchronize()
    got_bits = lb.unpack_packed(packed.cpu().numpy(), subfp_len)
    got_haar = haar.cpu().numpy()
    for i, name in enumerate(cases):
        want_haar, want_bits = want[name]
        assert np.array_equal(got_haar[i], want_haar, equal_nan=True), f"{name}: Haar differs ({form}, keep {keep})"
        # (a NaN's sign and payload are not comparable, and need not be: its sign code is 0 whatever they are, and it outranks
        # every other key)
        assert np.array_equal(got_bits[i], want_bits), f"{name}: bits differ ({form}, keep {keep})"


def test_cases_have_the_occupancy_they_claim(oracle):
    """The frames' own checks, without a device: the compile-time sparse form's bands and the general forms, as the device test
    builds them."""
    _, lo, hi = oracle.band_table(44100, 1024)
    for live, seed in ((np.asarray(lo) < np.asarray(hi), 1000), (np.ones(16, bool), 1002), (np.ones(32, bool), 1003), (np.ones(64, bool), 1004)):
        for subfp_len in (1, 200, 255):
            keep = (subfp_len + 1) // 2
            reference(oracle, build_cases(oracle, live, keep, seed), keep, subfp_len)


# ---- the compiled kernels' resources ---------------------------------------------------------------------------------
HIPCC = "/opt/rocm/bin/hipcc"
# LDS bytes of every instance before the bucket ranking: <COLS, SPARSE>
LDS_BEFORE = {("32", "1"): 15216, ("16", "0"): 12016, ("32", "0"): 22256, ("64", "0"): 42736}


def test_stage2_instances_keep_their_occupancy(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("no hipcc")
    out = tmp_path / "k_haar_select32.s"
    csrc = os.path.join(ROOT, "lbaudiodetective_amd", "csrc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fhip-fp32-correctly-rounded-divide-sqrt",
           "-mllvm", "-amdgpu-atomic-optimizer-strategy=None", "-x", "hip", "--cuda-device-only", "-S",
           "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "k_haar_select32.hip"), "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    isa = out.read_text()
    seen = 0
    for block in re.findall(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S):
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        m = re.search(r"haar_select32_kernelILi(\d+)ELb([01])E", name)
        assert m, name
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))     # noqa: E731
        assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0, (name, block)
        assert field("group_segment_fixed_size") <= LDS_BEFORE[m.groups()], name
        if m.group(2) == "1":
            assert field("vgpr_count") <= 64, (name, field("vgpr_count"))
        seen += 1
    assert seen == 5, seen
