"""Python mirror of the LBAudioDetective C interface over liblbaudiodetective.so.

Class and method names follow the upstream functions (``LBAudioDetectiveFingerprintCompareToFingerprint``
-> ``Fingerprint.compare_to_fingerprint``), argument meaning and error behaviour are the C
library's.  Everything that computes goes through the C ABI into HIP kernels; this module only
marshals buffers (numpy on the host, ``torch`` tensors for device memory and streams).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _native as N

noErr = 0


class LBAudioDetectiveError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        code = status & 0xFFFFFFFF
        four = bytes([(code >> s) & 0xFF for s in (24, 16, 8, 0)])
        tag = f"'{four.decode()}'" if all(32 <= b < 127 for b in four) else str(status)
        super().__init__(f"{what}: OSStatus {tag}")


def _check(status: int, what: str):
    if status != noErr:
        raise LBAudioDetectiveError(status, what)


def _u8(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint8)


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _stream_ptr(stream=None):
    """hipStream_t of a torch stream (default: torch's current stream; None without torch)."""
    if stream is not None:
        return C.c_void_p(stream.cuda_stream)
    try:
        import torch
        if torch.cuda.is_available():
            return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    except ImportError:
        pass
    return C.c_void_p(0)


def pack_subfingerprint(bools) -> np.ndarray:
    b = _u8(bools)
    out = np.zeros(N.PACKED_WORDS, np.uint32)
    N.lib().LBAudioDetectivePackSubfingerprint(b.ctypes.data, b.size, out.ctypes.data)
    return out


def unpack_subfingerprint(words, length: int) -> np.ndarray:
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(length, np.uint8)
    N.lib().LBAudioDetectiveUnpackSubfingerprint(w.ctypes.data, length, out.ctypes.data)
    return out


def unpack_packed(packed: np.ndarray, length: int) -> np.ndarray:
    """[..., 8] uint32 (or [..., 32] uint8) packed sub-fingerprints -> [..., length] Booleans."""
    p = np.ascontiguousarray(packed)
    if p.dtype == np.uint8:
        p = p.view(np.uint32)
    p = p.reshape(-1, N.PACKED_WORDS)
    bits = ((p[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).astype(np.uint8)
    return bits.reshape(p.shape[0], 256)[:, :length]


class Fingerprint:
    """LBAudioDetectiveFingerprintRef."""

    def __init__(self, subfingerprint_length: int = 0, _ref=None):
        self._L = N.lib()
        self._ref = _ref if _ref is not None else self._L.LBAudioDetectiveFingerprintNew(subfingerprint_length)

    @classmethod
    def from_bools(cls, bools) -> "Fingerprint":
        b = _u8(bools)
        assert b.ndim == 2
        fp = cls(b.shape[1])
        for row in b:
            fp.add_subfingerprint(row)
        return fp

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveFingerprintDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def copy(self) -> "Fingerprint":
        return Fingerprint(_ref=self._L.LBAudioDetectiveFingerprintCopy(self._ref))

    @property
    def subfingerprint_length(self) -> int:
        return self._L.LBAudioDetectiveFingerprintGetSubfingerprintLength(self._ref)

    @property
    def number_of_subfingerprints(self) -> int:
        return self._L.LBAudioDetectiveFingerprintGetNumberOfSubfingerprints(self._ref)

    def subfingerprint_at_index(self, index: int) -> np.ndarray:
        out = np.zeros(self.subfingerprint_length, np.uint8)
        self._L.LBAudioDetectiveFingerprintGetSubfingerprintAtIndex(self._ref, index, out.ctypes.data)
        return out

    def set_subfingerprint_length(self, length: int):
        io = N.UInt32(length)
        ok = self._L.LBAudioDetectiveFingerprintSetSubfingerprintLength(self._ref, C.byref(io))
        return bool(ok), io.value

    def add_subfingerprint(self, bools):
        b = _u8(bools)
        assert b.size >= self.subfingerprint_length
        self._L.LBAudioDetectiveFingerprintAddSubfingerprint(self._ref, b.ctypes.data)

    def equal_to_fingerprint(self, other: "Fingerprint") -> bool:
        return bool(self._L.LBAudioDetectiveFingerprintEqualToFingerprint(self._ref, other._ref))

    def compare_to_fingerprint(self, other: "Fingerprint", range_: int) -> float:
        return float(self._L.LBAudioDetectiveFingerprintCompareToFingerprint(self._ref, other._ref, range_))

    def compare_subfingerprints(self, a, b, range_: int) -> float:
        a, b = _u8(a), _u8(b)
        return float(self._L.LBAudioDetectiveFingerprintCompareSubfingerprints(self._ref, a.ctypes.data, b.ctypes.data,
                                                                                range_))

    def to_bools(self) -> np.ndarray:
        n, L = self.number_of_subfingerprints, self.subfingerprint_length
        out = np.zeros((n, L), np.uint8)
        for i in range(n):
            out[i] = self.subfingerprint_at_index(i)
        return out

    def to_string(self) -> str:
        """'0'/'1' per Boolean, sub-fingerprints joined by '+' (LBAudioDetectiveTests.m:22-37)."""
        n = int(self._L.LBAudioDetectiveFingerprintGetStringLength(self._ref))
        buf = C.create_string_buffer(n + 1)
        self._L.LBAudioDetectiveFingerprintGetString(self._ref, buf, n + 1)
        return buf.value.decode()

    @classmethod
    def from_string(cls, text: str) -> "Fingerprint":
        ref = N.lib().LBAudioDetectiveFingerprintNewFromString(text.encode())
        if not ref:
            raise ValueError("malformed fingerprint string")
        return cls(_ref=ref)


class Frame:
    """LBAudioDetectiveFrameRef."""

    def __init__(self, max_row_count: int, _ref=None):
        self._L = N.lib()
        self._ref = _ref if _ref is not None else self._L.LBAudioDetectiveFrameNew(max_row_count)

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveFrameDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def copy(self) -> "Frame":
        return Frame(0, _ref=self._L.LBAudioDetectiveFrameCopy(self._ref))

    @property
    def number_of_rows(self) -> int:
        return self._L.LBAudioDetectiveFrameGetNumberOfRows(self._ref)

    def full(self) -> bool:
        return bool(self._L.LBAudioDetectiveFrameFull(self._ref))

    def set_row(self, row, index: int) -> bool:
        r = _f32(row)
        return bool(self._L.LBAudioDetectiveFrameSetRow(self._ref, r.ctypes.data, index, r.size))

    def get_value(self, row: int, col: int) -> float:
        return float(self._L.LBAudioDetectiveFrameGetValue(self._ref, row, col))

    def get_row(self, index: int, count: int) -> np.ndarray:
        p = self._L.LBAudioDetectiveFrameGetRow(self._ref, index)
        return np.ctypeslib.as_array(p, shape=(count,)).copy()

    def decompose(self):
        self._L.LBAudioDetectiveFrameDecompose(self._ref)

    def fingerprint_length(self) -> int:
        return self._L.LBAudioDetectiveFrameFingerprintLength(self._ref)

    def fingerprint_size(self) -> int:
        return self._L.LBAudioDetectiveFrameFingerprintSize(self._ref)

    def extract_fingerprint(self, n_wavelets: int) -> np.ndarray:
        out = np.zeros(2 * n_wavelets, np.uint8)
        self._L.LBAudioDetectiveFrameExtractFingerprint(self._ref, n_wavelets, out.ctypes.data)
        return out

    def equal_to_frame(self, other: "Frame") -> bool:
        return bool(self._L.LBAudioDetectiveFrameEqualToFrame(self._ref, other._ref))


class Detective:
    """LBAudioDetectiveRef."""

    def __init__(self):
        self._L = N.lib()
        self._ref = self._L.LBAudioDetectiveNew()

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    # getters / setters (D.h:74-205)
    processing_sample_rate = property(
        lambda s: s._L.LBAudioDetectiveGetProcessingSampleRate(s._ref),
        lambda s, v: _check(s._L.LBAudioDetectiveSetProcessingSampleRate(s._ref, float(v)), "SetProcessingSampleRate"))
    number_of_pitch_steps = property(
        lambda s: s._L.LBAudioDetectiveGetNumberOfPitchSteps(s._ref),
        lambda s, v: _check(s._L.LBAudioDetectiveSetNumberOfPitchSteps(s._ref, int(v)), "SetNumberOfPitchSteps"))
    subfingerprint_length = property(
        lambda s: s._L.LBAudioDetectiveGetSubfingerprintLength(s._ref),
        lambda s, v: _check(s._L.LBAudioDetectiveSetSubfingerprintLength(s._ref, int(v)), "SetSubfingerprintLength"))
    window_size = property(
        lambda s: s._L.LBAudioDetectiveGetWindowSize(s._ref),
        lambda s, v: _check(s._L.LBAudioDetectiveSetWindowSize(s._ref, int(v)), "SetWindowSize"))
    analysis_stride = property(
        lambda s: s._L.LBAudioDetectiveGetAnalysisStride(s._ref),
        lambda s, v: _check(s._L.LBAudioDetectiveSetAnalysisStride(s._ref, int(v)), "SetAnalysisStride"))

    def set_window_size_status(self, v: int) -> int:
        return self._L.LBAudioDetectiveSetWindowSize(self._ref, int(v))

    def configure(self, sample_rate=None, window=None, stride=None, bands=None, subfp_len=None) -> "Detective":
        if sample_rate is not None:
            self.processing_sample_rate = sample_rate
        if window is not None:
            self.window_size = window
        if stride is not None:
            self.analysis_stride = stride
        if bands is not None:
            self.number_of_pitch_steps = bands
        if subfp_len is not None:
            self.subfingerprint_length = subfp_len
        return self

    def set_file_pipeline(self, enabled: bool):
        """Two runs of a file batch in flight (default) or one at a time (LBAudioDetectiveSetFilePipeline)."""
        _check(self._L.LBAudioDetectiveSetFilePipeline(self._ref, 1 if enabled else 0), "SetFilePipeline")
        return self

    def set_kernel_variant(self, variant: int):
        _check(self._L.LBAudioDetectiveSetKernelVariant(self._ref, variant), "SetKernelVariant")

    def set_band_sum_form(self, form: int):
        """Band sums of the pruned stage 1: 0 automatic, 1 through LDS, 2 in lanes (an error where the settings have no such form)."""
        _check(self._L.LBAudioDetectiveSetBandSumForm(self._ref, form), "SetBandSumForm")

    def band_sum_form(self) -> int:
        """The form (1 or 2) a call under the present settings would take."""
        form = N.UInt32(0)
        _check(self._L.LBAudioDetectiveGetBandSumForm(self._ref, C.byref(form)), "GetBandSumForm")
        return int(form.value)

    def set_scratch_limit(self, n_bytes: int):
        _check(self._L.LBAudioDetectiveSetScratchLimit(self._ref, n_bytes), "SetScratchLimit")

    def set_stage_timing(self, enabled: bool):
        _check(self._L.LBAudioDetectiveSetStageTiming(self._ref, int(enabled)), "SetStageTiming")

    def stage_times(self):
        """(stage 1 ms, stage 2 ms, launches per stage) of the last batch call; waits for it."""
        a, b, n = N.Float32(0), N.Float32(0), N.UInt32(0)
        _check(self._L.LBAudioDetectiveGetStageTimes(self._ref, C.byref(a), C.byref(b), C.byref(n)), "GetStageTimes")
        return float(a.value), float(b.value), int(n.value)

    def subfingerprint_count(self, n_samples: int) -> int:
        return int(self._L.LBAudioDetectiveGetSubfingerprintCount(self._ref, n_samples))

    def set_kernel_tuning(self, waves_per_workgroup: int = 0, twiddle_cache: bool = True):
        """Measurement knobs of the generic stage-1 kernel (tools/sweep_lds_tiles.py)."""
        _check(self._L.LBAudioDetectiveSetKernelTuning(self._ref, waves_per_workgroup, int(twiddle_cache)), "SetKernelTuning")
        return self

    def set_file_hop_mode(self, mode: int):
        """1 (default): upstream's file-frame hop; 0: hop in processing-rate samples."""
        _check(self._L.LBAudioDetectiveSetFileHopMode(self._ref, mode), "SetFileHopMode")
        return self

    def set_file_tail_mode(self, mode: int):
        """Hop mode 1, windows reaching past the end of the file: 1 (default) nothing is read -> zero rows,
        2 partial reads over the stale spectrum, 0 zero-filled."""
        _check(self._L.LBAudioDetectiveSetFileTailMode(self._ref, mode), "SetFileTailMode")
        return self

    def set_resampler_mode(self, mode: int):
        """0 (default) long Kaiser sinc, 1 short sinc, 2 linear interpolation."""
        _check(self._L.LBAudioDetectiveSetResamplerMode(self._ref, mode), "SetResamplerMode")
        return self

    def process_file_stream(self, client_samples, file_frames: int, hop: int) -> "Fingerprint":
        """Upstream's file loop (D.m:241-293) on a file already converted to the processing rate."""
        x = _f32(client_samples).reshape(-1)
        out = N.Ref()
        _check(self._L.LBAudioDetectiveProcessFileStream(self._ref, x.ctypes.data, x.size, int(file_frames), int(hop),
                                                         C.byref(out)), "ProcessFileStream")
        return Fingerprint(_ref=out.value)

    # file entry points (D.h:218,235)
    def process_audio_url(self, path: str) -> Fingerprint:
        out = N.Ref()
        _check(self._L.LBAudioDetectiveProcessAudioURL(self._ref, path.encode(), C.byref(out)), "ProcessAudioURL")
        return Fingerprint(_ref=out.value)

    def process_audio_urls(self, paths, statuses: bool = False):
        """LBAudioDetectiveProcessAudioURLs: every file through one launch chain -> list of Fingerprint (None where a
        file failed; with statuses=True also the list of OSStatus values, else a failure raises)."""
        n = len(paths)
        arr = (C.c_char_p * n)(*[p.encode() for p in paths])
        refs = (N.Ref * n)()
        sts = (N.OSStatus * n)()
        _check(self._L.LBAudioDetectiveProcessAudioURLs(self._ref, arr, n, refs, sts), "ProcessAudioURLs")
        fps = [Fingerprint(_ref=refs[i]) if refs[i] else None for i in range(n)]
        if statuses:
            return fps, [int(sts[i]) for i in range(n)]
        for i in range(n):
            _check(int(sts[i]), f"ProcessAudioURLs[{paths[i]}]")
        return fps

    def convert_audio_url(self, path: str):
        """The device front end alone: (mono samples at the processing rate, file frames, file rate)."""
        buf, n, ff, rate = C.POINTER(N.Float32)(), N.UInt64(0), N.UInt64(0), N.Float64(0.0)
        _check(self._L.LBAudioDetectiveConvertAudioURL(self._ref, path.encode(), C.byref(buf), C.byref(n), C.byref(ff),
                                                       C.byref(rate)), "ConvertAudioURL")
        try:
            out = np.ctypeslib.as_array(buf, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
        finally:
            self._L.LBAudioDetectiveFreeSamples(buf)
        return out, int(ff.value), float(rate.value)

    def compare_audio_urls(self, path1: str, path2: str, range_: int = 0) -> float:
        m = N.Float32(float("nan"))
        _check(self._L.LBAudioDetectiveCompareAudioURLs(self._ref, path1.encode(), path2.encode(), range_, C.byref(m)),
               "CompareAudioURLs")
        return float(m.value)

    # PCM entry points
    def process_pcm(self, pcm) -> Fingerprint:
        x = _f32(pcm).reshape(-1)
        out = N.Ref()
        _check(self._L.LBAudioDetectiveProcessPCM(self._ref, x.ctypes.data, x.size, C.byref(out)), "ProcessPCM")
        return Fingerprint(_ref=out.value)

    def compare_pcm(self, pcm1, pcm2, range_: int = 0) -> float:
        a, b = _f32(pcm1).reshape(-1), _f32(pcm2).reshape(-1)
        m = N.Float32(float("nan"))
        _check(self._L.LBAudioDetectiveComparePCM(self._ref, a.ctypes.data, a.size, b.ctypes.data, b.size, range_,
                                                  C.byref(m)), "ComparePCM")
        return float(m.value)

    def fingerprint_clips(self, clips) -> np.ndarray:
        """Host batch: [n_clips, samples] float32 (or int16 / int32 PCM) -> [n_clips, count, subfp_len] Booleans."""
        x = np.asarray(clips)
        fmt = {np.dtype(np.int16): 1, np.dtype(np.int32): 2}.get(x.dtype, 0)
        x = np.ascontiguousarray(x) if fmt else _f32(x)
        n, spc = x.shape
        per = self.subfingerprint_count(spc)
        out = np.zeros((n, per, self.subfingerprint_length), np.uint8)
        _check(self._L.LBAudioDetectiveFingerprintClipsFormat(self._ref, x.ctypes.data, fmt, n, spc, out.ctypes.data),
               "FingerprintClips")
        return out

    def fingerprint_clips_device(self, clips, out=None, stream=None, taps: bool = False):
        """Device batch on torch tensors: clips [n, samples] float32 (cuda) -> packed uint8 [n, count, 32].

        Asynchronous on the given (default: current) torch stream.  With taps=True also returns the
        128 x bands frames before and after the Haar (full rows between the stages).  int16 / int32 PCM is taken as well."""
        import torch
        assert clips.is_cuda and clips.is_contiguous() and clips.dtype in (torch.float32, torch.int16, torch.int32)
        n, spc = clips.shape
        per = self.subfingerprint_count(spc)
        if out is None:
            out = torch.empty((n, per, N.PACKED_BYTES), dtype=torch.uint8, device=clips.device)
        sp = _stream_ptr(stream)
        fmt = {torch.float32: 0, torch.int16: 1, torch.int32: 2}[clips.dtype]
        if not taps:
            _check(self._L.LBAudioDetectiveFingerprintClipsDeviceFormat(self._ref, clips.data_ptr(), fmt, n, spc,
                                                                       out.data_ptr(), sp), "FingerprintClipsDevice")
            return out
        bands = self.number_of_pitch_steps
        raw = torch.empty((n, per, N.ROWS_PER_FRAME, bands), dtype=torch.float32, device=clips.device)
        haar = torch.empty_like(raw)
        _check(self._L.LBAudioDetectiveFingerprintClipsDeviceTapsFormat(self._ref, clips.data_ptr(), fmt, n, spc, out.data_ptr(),
                                                                       raw.data_ptr(), haar.data_ptr(), sp),
               "FingerprintClipsDeviceTapsFormat")
        return out, raw, haar

    def subfingerprint_count_at_phase(self, n_samples: int, phases: int, phase: int) -> int:
        """Sub-fingerprints of phase `phase` of `phases` (1, 2, 4, ... 32) of a signal of n_samples: the count of the signal without
        its first phase_sample_offset(phases, phase, stride) samples; 0 for a phase count or phase that does not exist."""
        return int(self._L.LBAudioDetectiveGetSubfingerprintCountAtPhase(self._ref, n_samples, phases, phase))

    def fingerprint_clips_device_phases(self, clips, phases: int, out=None, stream=None):
        """The device batch at `phases` frame phases: clips [n, samples] (cuda; float32, int16 or int32) -> uint32
        [n, phases, count_0, 8], row (c, p) the packed sub-fingerprints of clip c without its first
        phase_sample_offset(phases, p, stride) samples, zero at and behind subfingerprint_count_at_phase(samples, phases, p).
        The windows of a clip are transformed once whatever `phases`.  Asynchronous on the given (default: current) stream."""
        import torch
        assert clips.is_cuda and clips.is_contiguous() and clips.dtype in (torch.float32, torch.int16, torch.int32)
        n, spc = clips.shape
        per = self.subfingerprint_count(spc)
        if out is None:
            out = torch.empty((n, int(phases), per, N.PACKED_WORDS), dtype=torch.int32, device=clips.device).view(torch.uint32)
        assert out.is_cuda and out.is_contiguous() and out.numel() * out.element_size() >= n * int(phases) * per * N.PACKED_BYTES
        fmt = {torch.float32: 0, torch.int16: 1, torch.int32: 2}[clips.dtype]
        _check(self._L.LBAudioDetectiveFingerprintClipsDevicePhases(self._ref, clips.data_ptr(), fmt, n, spc, int(phases), out.data_ptr(),
                                                                   _stream_ptr(stream)), "FingerprintClipsDevicePhases")
        return out

    def stage1_choice(self, fmt: int, n_clips: int, samples_per_clip: int, address: int = 0, taps: bool = False,
                      tail: bool = False, variant: int = 0, waves: int = 0, cache: bool = True) -> "Stage1Choice":
        """debug_stage1_choice for this detective's settings; variant and tuning are not readable from the handle and are
        given as they were set."""
        return debug_stage1_choice(self.processing_sample_rate, self.window_size, self.analysis_stride, self.number_of_pitch_steps,
                                   self.subfingerprint_length, variant, waves, cache, fmt, n_clips, samples_per_clip, address % 8,
                                   taps, tail)


def phase_sample_offset(phases: int, phase: int, stride: int) -> int:
    """First sample of frame phase `phase` of `phases`: phase * (128 / phases) * stride.  Sub-fingerprint j of that phase starts
    phase_sample_offset(...) + j * 128 * stride samples into the signal."""
    phases, phase = int(phases), int(phase)
    if phases not in (1, 2, 4, 8, 16, 32) or not 0 <= phase < phases:
        raise ValueError(f"no phase {phase} of {phases}")
    return phase * (N.ROWS_PER_FRAME // phases) * int(stride)


STAGE1_FAMILIES = ("generic", "pruned", "stream2", "full", "stream")
STAGE2_FAMILIES = ("generic", "select32", "select32_sparse")
Stage1Choice = collections.namedtuple("Stage1Choice", "status launches family args compact stage2 fell_back per words")


def debug_stage1_choice(sample_rate: float, window: int, stride: int, bands: int, subfp_len: int, variant: int = 0, waves: int = 0,
                        cache: bool = True, fmt: int = 0, n_clips: int = 1, samples_per_clip: int = 0, address_mod8: int = 0,
                        taps: bool = False, tail: bool = False) -> "Stage1Choice":
    """LBAudioDetectiveDebugStage1Choice (tests): the kernels one batch call takes, from the header's 12 words.  Needs no GPU.
    family / stage2: names of STAGE1_FAMILIES / STAGE2_FAMILIES (None when nothing is launched); args: the instance's template
    arguments -- generic (LOG2W, WPB, CACHED), pruned (FMT,), stream2 (FMT, QLO, QHI), full (LOG2L, FMT, S64, lean), stream (FMT,);
    fell_back: the tuning asked for was not taken; status: what the call would return."""
    out = (N.UInt32 * 12)()
    _check(N.lib().LBAudioDetectiveDebugStage1Choice(float(sample_rate), window, stride, bands, subfp_len, variant, waves, int(cache),
                                                     fmt, n_clips, samples_per_clip, address_mod8, int(taps), int(tail), out, 12),
           "DebugStage1Choice")
    w = [int(x) for x in out]
    status = w[0] - (1 << 32) if w[0] >= (1 << 31) else w[0]
    if not w[1]:
        return Stage1Choice(status, False, None, (), False, None, False, 0, w)
    family = STAGE1_FAMILIES[w[2]]
    n_args = {"generic": 3, "pruned": 1, "stream2": 3, "full": 4, "stream": 1}[family]
    return Stage1Choice(status, True, family, tuple(w[3:3 + n_args]), bool(w[7]), STAGE2_FAMILIES[w[8]], bool(w[9] or w[10]), w[11], w)


def compact_layout(det: "Detective"):
    """(live band among bands 0..15 or 32, columns of the row transform that can be non-zero) of the configuration's compact
    inter-stage frames, or None when it has none (LBAudioDetectiveGetCompactLayout)."""
    left, cols = N.UInt32(0), N.UInt32(0)
    st = N.lib().LBAudioDetectiveGetCompactLayout(det._ref, C.byref(left), C.byref(cols))
    return (int(left.value), int(cols.value)) if st == 0 else None


def compact_bands(det: "Detective"):
    """The bands a row of a compact inter-stage frame holds, in storage order (LBAudioDetectiveGetCompactBands), or None."""
    bands, count = (N.UInt32 * 17)(), N.UInt32(0)
    st = N.lib().LBAudioDetectiveGetCompactBands(det._ref, bands, C.byref(count))
    return [int(bands[i]) for i in range(count.value)] if st == 0 else None


def frames_to_subfingerprints_device(det: "Detective", frames, want_haar: bool = False, stream=None, compact: bool = False):
    """Stage 2 alone on torch frames [n, 128, bands] float32 (cuda) -> packed uint8 [n, 32] (and the Haar frames).
    compact: through the SPARSE form -- the frames (whose structurally empty bands must be zero) are packed into the
    compact layout first (128 rows of the bands that can be non-zero)."""
    import torch
    assert frames.is_cuda and frames.dtype == torch.float32 and frames.is_contiguous()
    n = frames.shape[0]
    out = torch.empty((n, N.PACKED_BYTES), dtype=torch.uint8, device=frames.device)
    haar = torch.empty_like(frames) if want_haar else None
    if compact:
        lay = compact_layout(det)
        if lay is None:
            raise LBAudioDetectiveError(1, "this configuration has no compact frame layout")
        cf = frames[:, :, compact_bands(det)].contiguous()          # [n, 128, stored bands]
        _check(N.lib().LBAudioDetectiveCompactFramesToSubfingerprintsDevice(det._ref, cf.data_ptr(), n, out.data_ptr(),
                                                                            haar.data_ptr() if want_haar else None, _stream_ptr(stream)),
               "CompactFramesToSubfingerprintsDevice")
        return (out, haar) if want_haar else out
    _check(N.lib().LBAudioDetectiveFramesToSubfingerprintsDevice(det._ref, frames.data_ptr(), n, out.data_ptr(),
                                                                 haar.data_ptr() if want_haar else None, _stream_ptr(stream)),
           "FramesToSubfingerprintsDevice")
    return (out, haar) if want_haar else out


class Stream:
    """LBAudioDetectiveStreamRef: chunked PCM in, partial frame carried across calls."""

    def __init__(self, detective: Detective):
        self._L = N.lib()
        self._det = detective            # keep the detective alive
        self._ref = self._L.LBAudioDetectiveStreamNew(detective._ref)

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveStreamDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def push(self, samples) -> int:
        x = _f32(samples).reshape(-1)
        new = N.UInt32(0)
        _check(self._L.LBAudioDetectiveStreamPush(self._ref, x.ctypes.data, x.size, C.byref(new)), "StreamPush")
        return int(new.value)

    def fingerprint(self) -> Fingerprint:
        return Fingerprint(_ref=self._L.LBAudioDetectiveStreamCopyFingerprint(self._ref))


def _u32_list(values):
    a = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.uint32)
    return a, (a.ctypes.data_as(C.POINTER(N.UInt32)) if a.size else None)


def debug_stream_bank_plan(window: int, stride: int, history: int, pending, counts):
    """LBAudioDetectiveDebugStreamBankPlan (tests): the host plan of one push -> (ready, pending_after, kept), uint32 arrays with
    one value per channel.  Needs no GPU."""
    p, pp = _u32_list(pending)
    n, np_ = _u32_list(counts)
    if p.size != n.size:
        raise ValueError("pending and counts must have one value per channel")
    out = [np.zeros(max(1, p.size), np.uint32) for _ in range(3)]
    _check(N.lib().LBAudioDetectiveDebugStreamBankPlan(window, stride, history, p.size, pp, np_,
                                                       *[o.ctypes.data_as(C.POINTER(N.UInt32)) for o in out]), "DebugStreamBankPlan")
    return tuple(o[:p.size] for o in out)


class StreamBank:
    """LBAudioDetectiveStreamBankRef: `n_channels` live channels whose carried partial frames and `history` most recent
    sub-fingerprints stay on the device.  A push takes new samples of any of the channels and fingerprints every frame they
    complete in one launch chain; `window_device` hands the most recent sub-fingerprints of some channels to the packed queries.
    frames_per_pass bounds the staging memory (0: one frame per channel); results do not depend on it.

    phases given (1, 2, 4, ... 32; 1 included) makes a PHASED bank (LBAudioDetectiveStreamBankNewPhased): n_channels * phases
    virtual channels, virtual(c, p) holding the sub-fingerprints of channel c's samples without the first
    phase_sample_offset(phases, p, stride) -- every frame grid `128 / phases` rows apart, from ONE transform of the channel's
    windows.  Pushes and reset take the real channels; new counts, totals, window_device, fingerprint and every query built on
    window_device take virtual channel indices.  Without `phases` the bank is the unphased one (LBAudioDetectiveStreamBankNew),
    as it always was: `phases` and `virtual_channels` then read 1 and n_channels, `phased` False."""

    def __init__(self, detective: Detective, n_channels: int, history: int, frames_per_pass: int = 0, phases: int = None):
        self._L = N.lib()
        self._det = detective            # keep the detective alive
        self.n_channels, self.history = int(n_channels), int(history)
        self.phased = phases is not None
        self.phases = int(phases) if self.phased else 1
        self.virtual_channels = self.n_channels * self.phases
        if self.phased:
            self._ref = self._L.LBAudioDetectiveStreamBankNewPhased(detective._ref, n_channels, history, frames_per_pass, self.phases)
        else:
            self._ref = self._L.LBAudioDetectiveStreamBankNew(detective._ref, n_channels, history, frames_per_pass)
        if not self._ref:
            raise LBAudioDetectiveError(1, "StreamBankNewPhased" if self.phased else "StreamBankNew")

    def virtual(self, channel: int, phase: int = 0) -> int:
        """The virtual channel of (channel, phase): channel * phases + phase."""
        if not 0 <= channel < self.n_channels or not 0 <= phase < self.phases:
            raise IndexError(f"(channel {channel}, phase {phase}) of a bank of {self.n_channels} x {self.phases}")
        return channel * self.phases + phase

    def work(self):
        """LBAudioDetectiveStreamBankGetWork (a phased bank): (windows transformed, frames selected) since creation."""
        w, f = N.UInt64(0), N.UInt64(0)
        _check(self._L.LBAudioDetectiveStreamBankGetWork(self._ref, C.byref(w), C.byref(f)), "StreamBankGetWork")
        return int(w.value), int(f.value)

    def _new_room(self, n) -> int:
        """room for the sub-fingerprints a push of n samples per channel completes: their number for an unphased bank (the host
        can tell alone); for a phased bank a bound, n / (128 stride) + 1 per virtual channel -- _push hands back the filled part"""
        if not self.phased:
            return int(debug_stream_bank_plan(self._det.window_size, self._det.analysis_stride, self.history, self.pending(), n)[0].sum())
        hop = N.ROWS_PER_FRAME * self._det.analysis_stride
        return sum(self.phases * (int(x) // hop + 1) for x in n if x)

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveStreamBankDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def _push(self, fn, what, samples_ptr, counts, new_out, stream, device):
        n, npt = _u32_list(counts)
        if n.size != self.n_channels:
            raise ValueError("counts must have one value per channel")
        if new_out is True:              # sized from the plan, which the host can make alone
            import torch
            new_out = torch.empty((self._new_room(n), N.PACKED_BYTES), dtype=torch.uint8, device=device)
        capacity = 0
        if new_out is not None:
            if not new_out.is_cuda or not new_out.is_contiguous():
                raise ValueError("new_out must be a contiguous device tensor")
            capacity = new_out.numel() * new_out.element_size() // N.PACKED_BYTES
        new_counts = np.zeros(self.virtual_channels, np.uint32)
        total = N.UInt64(0)
        _check(fn(self._ref, samples_ptr, npt, new_counts.ctypes.data_as(C.POINTER(N.UInt32)),
                  _dev_ptr(new_out) if new_out is not None and new_out.numel() else None, capacity, C.byref(total), _stream_ptr(stream)), what)
        if new_out is None:
            return new_counts, None
        import torch
        return new_counts, new_out.view(torch.uint8).reshape(-1, N.PACKED_BYTES)[:total.value]

    def push_device(self, samples, counts, new_out=None, stream=None):
        """LBAudioDetectiveStreamBankPushDevice: `samples`, a float32 device tensor holding the channels' new samples one after
        the other in channel order; `counts`, one host integer per channel.  new_out: None, True (a tensor for the new
        sub-fingerprints is made) or a contiguous device tensor with room for them -> (new_counts uint32 [virtual_channels] on the
        host -- [n_channels] for an unphased bank --, the new sub-fingerprints uint8 [total, 32] on the device in (virtual) channel
        order then time order, or None).  Asynchronous on
        `stream`; `samples` must stay untouched until the stream has run the call."""
        import torch
        assert samples.is_cuda and samples.is_contiguous() and samples.dtype == torch.float32
        if samples.numel() < int(np.asarray(counts, dtype=np.uint64).sum()):
            raise ValueError("samples holds fewer values than the counts add up to")
        return self._push(self._L.LBAudioDetectiveStreamBankPushDevice, "StreamBankPushDevice",
                          C.c_void_p(samples.data_ptr()) if samples.numel() else None, counts, new_out, stream, samples.device)

    def push(self, chunks, new_out=None, stream=None):
        """LBAudioDetectiveStreamBankPush: `chunks`, one numpy array of new samples per channel (None or empty: nothing for that
        channel), from host memory; returns as push_device once the samples have been taken."""
        if len(chunks) != self.n_channels:
            raise ValueError("chunks must have one entry per channel")
        parts = [_f32(c).reshape(-1) if c is not None else np.zeros(0, np.float32) for c in chunks]
        x = np.concatenate(parts) if parts else np.zeros(0, np.float32)
        return self._push(self._L.LBAudioDetectiveStreamBankPush, "StreamBankPush", C.c_void_p(x.ctypes.data) if x.size else None,
                          [p.size for p in parts], new_out, stream, "cuda")

    def totals(self) -> np.ndarray:
        """sub-fingerprints of every channel since creation / its last reset (uint64, the host mirror)"""
        out = np.zeros(self.virtual_channels, np.uint64)
        _check(self._L.LBAudioDetectiveStreamBankGetCounts(self._ref, out.ctypes.data_as(C.POINTER(N.UInt64)), None), "StreamBankGetCounts")
        return out

    def pending(self) -> np.ndarray:
        """samples every channel carries (uint32, the host mirror)"""
        out = np.zeros(self.n_channels, np.uint32)
        _check(self._L.LBAudioDetectiveStreamBankGetCounts(self._ref, None, out.ctypes.data_as(C.POINTER(N.UInt32))), "StreamBankGetCounts")
        return out

    def window_device(self, channels, n: int, out=None, stream=None):
        """LBAudioDetectiveStreamBankWindowDevice: the n most recent sub-fingerprints of each listed channel, oldest first, as
        uint8 [len(channels), n, 32] on the device -- the `packed` of the ...packed..._device queries.  Asynchronous on `stream`."""
        ch, cp = _u32_list(channels)
        if out is None:
            import torch
            with torch.cuda.stream(stream):              # (the block belongs to the stream that fills it)
                out = torch.empty((ch.size, n, N.PACKED_BYTES), dtype=torch.uint8, device="cuda")
        if not out.is_cuda or not out.is_contiguous() or out.numel() * out.element_size() < ch.size * n * N.PACKED_BYTES:
            raise ValueError("out must be a contiguous device tensor of at least len(channels) * n * 32 bytes")
        _check(self._L.LBAudioDetectiveStreamBankWindowDevice(self._ref, cp, ch.size, n, _dev_ptr(out), _stream_ptr(stream)),
               "StreamBankWindowDevice")
        return out

    def fingerprint(self, channel: int) -> Fingerprint:
        """LBAudioDetectiveStreamBankCopyFingerprint: the min(total, history) most recent sub-fingerprints of one channel."""
        if not 0 <= channel < self.virtual_channels:
            raise IndexError(f"channel {channel} of a bank of {self.virtual_channels}")
        ref = self._L.LBAudioDetectiveStreamBankCopyFingerprint(self._ref, channel)
        if not ref:
            raise LBAudioDetectiveError(1, "StreamBankCopyFingerprint")
        return Fingerprint(_ref=ref)

    def reset(self, channels):
        """LBAudioDetectiveStreamBankResetChannels: the listed channels start again."""
        ch, cp = _u32_list(channels)
        _check(self._L.LBAudioDetectiveStreamBankResetChannels(self._ref, cp, ch.size), "StreamBankResetChannels")

    def identify(self, corpus: "Corpus", channels, n: int, k: int = 1, aligned: bool = False, range_: int = 0, stream=None):
        """The n most recent sub-fingerprints of the listed channels against the corpus: window_device, then
        Corpus.query_packed_topk_keys_device on its output, on ONE stream with nothing in between.  Returns the [len(channels), k]
        int64 key tensor, and with aligned=True (keys, lags int32)."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_topk_keys_device(packed, packed.shape[0], n, k, aligned=aligned, range_=range_, stream=stream)

    def identify_recordings(self, corpus: "Corpus", channels, n: int, k: int = 1, aligned: bool = False, range_: int = 0,
                            index_base: int = 0, stream=None):
        """identify through the batch recording top-K: window_device, then Corpus.query_packed_recording_topk_batch_keys_device on
        its output, on ONE stream with nothing in between.  Returns what identify returns, bit for bit (a ragged corpus): the
        [len(channels), k] int64 key tensor, and with aligned=True (keys, lags int32) -- in entry-length steps per pair."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_recording_topk_batch_keys_device(packed, packed.shape[0], n, k, range_=range_, index_base=index_base,
                                                                    aligned=aligned, stream=stream)

    def timeline(self, corpus: "Corpus", channels, n: int, threshold: float, range_: int = 0, index_base: int = 0,
                 want_lengths: bool = True, stream=None):
        """What plays on every listed channel: the n most recent sub-fingerprints of each against the corpus, window_device, then
        Corpus.recording_timeline_batch_keys_device on its output, on ONE stream with nothing in between.  Returns (keys int64
        [len(channels), n], lengths int32 of the same shape or None): per channel and offset of its window the best entry at or
        above `threshold` that starts there and lies inside the window."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.recording_timeline_batch_keys_device(packed, packed.shape[0], n, threshold, range_=range_, index_base=index_base,
                                                           want_lengths=want_lengths, stream=stream)

    def segments(self, corpus: "Corpus", channels, n: int, threshold: float, capacity: int, range_: int = 0, index_base: int = 0,
                 stream=None):
        """What played when on every listed channel: window_device, then Corpus.recording_segments_batch_keys_device on its
        output, on ONE stream with nothing in between.  Returns (starts int32, keys int64, lengths int32, all [len(channels),
        capacity], counts int32 [len(channels)]): per channel the non-overlapping spans of its window of n sub-fingerprints in
        start order."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.recording_segments_batch_keys_device(packed, packed.shape[0], n, threshold, capacity, range_=range_,
                                                           index_base=index_base, stream=stream)

    def occurrences(self, corpus: "Corpus", channels, n: int, threshold: float, capacity: int, peaks: bool = True, range_: int = 0,
                    index_base: int = 0, want_lags: bool = True, stream=None):
        """Every place the window of every listed channel matches the corpus at or above `threshold`: window_device, then
        Corpus.query_packed_occurrences_batch_keys_device on its output, on ONE stream with nothing in between.  Returns (keys
        int64 [len(channels), capacity], lags int32 of the same shape or None, counts int64 [len(channels)]): per channel its
        matches in (entry, offset) order -- with peaks (the default) the local peaks of every profile only."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_occurrences_batch_keys_device(packed, packed.shape[0], n, threshold, capacity, peaks=peaks,
                                                                 range_=range_, index_base=index_base, want_lags=want_lags,
                                                                 stream=stream)

    def occurrence_segments(self, corpus: "Corpus", channels, n: int, threshold: float, capacity: int, out_capacity: int,
                            peaks: bool = True, range_: int = 0, index_base: int = 0, stream=None):
        """What played when on every listed channel, over ALL matching cells: window_device, then
        Corpus.recording_occurrence_segments_batch_keys_device on its output, on ONE stream with nothing in between.  Returns
        (starts int32, keys int64, lags int32, lengths int32, all [len(channels), out_capacity], counts int32 [len(channels)],
        occurrence_counts int64 [len(channels)]): per channel the non-overlapping spans of its window of n sub-fingerprints in
        start order, and the number of cells its occurrences row would hold -- above `capacity` the row was cut before the
        greedy ran."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.recording_occurrence_segments_batch_keys_device(packed, packed.shape[0], n, threshold, capacity, out_capacity,
                                                                      peaks=peaks, range_=range_, index_base=index_base, stream=stream)

    def new_occurrences(self, corpus: "Corpus", channels, n: int, new_counts, threshold: float, capacity: int, max_new: int = None,
                        range_: int = 0, index_base: int = 0, want_lags: bool = True, stream=None):
        """The matches the latest push completed on every listed channel: window_device, then
        Corpus.query_packed_occurrences_tail_batch_keys_device on its output, on ONE stream with nothing in between.  new_counts:
        what push / push_device returned (one value per channel of the BANK; the listed channels' are taken), or a device tensor
        with one value per LISTED channel (max_new required).  Returns (keys int64 [len(channels), capacity], lags int32 of the
        same shape or None, counts int64 [len(channels)]): per channel the cells at or above `threshold` whose entry ends inside
        the channel's new sub-fingerprints, in (entry, offset) order -- each match once in a channel's life as long as n >=
        the longest entry + the push's new sub-fingerprints - 1.  Decode with decode_tail_occurrences and totals()."""
        if not hasattr(new_counts, "data_ptr"):
            ch, _ = _u32_list(channels)
            new_counts = np.asarray(new_counts).reshape(-1)[ch]
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_occurrences_tail_batch_keys_device(packed, packed.shape[0], n, new_counts, threshold, capacity,
                                                                      max_new=max_new, range_=range_, index_base=index_base,
                                                                      want_lags=want_lags, stream=stream)

    def new_peaks(self, corpus: "Corpus", channels, n: int, new_counts, threshold: float, capacity: int, final: bool = False,
                  max_new: int = None, range_: int = 0, index_base: int = 0, want_lags: bool = True, stream=None):
        """One event per airing: the peaks among the cells the latest push made judgeable on every listed channel: window_device,
        then Corpus.query_packed_occurrences_tail_peaks_batch_keys_device on its output, on ONE stream with nothing in between.
        new_counts as new_occurrences takes them.  A cell is judged one sub-fingerprint late, when its right neighbour exists;
        final=True also judges the newest cell -- call it (new counts 0) at the end of a stream or before reset.  Returns (keys
        int64 [len(channels), capacity], lags int32 of the same shape or None, counts int64 [len(channels)]); each peak once in a
        channel's life as long as n >= the longest entry + the push's new sub-fingerprints + 1.  Decode with
        decode_tail_occurrences and totals()."""
        if not hasattr(new_counts, "data_ptr"):
            ch, _ = _u32_list(channels)
            new_counts = np.asarray(new_counts).reshape(-1)[ch]
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_occurrences_tail_peaks_batch_keys_device(packed, packed.shape[0], n, new_counts, threshold, capacity,
                                                                            max_new=max_new, final=final, range_=range_,
                                                                            index_base=index_base, want_lags=want_lags, stream=stream)

    def new_best(self, corpus: "Corpus", channels, n: int, new_counts, k: int = 1, max_new: int = None, aligned: bool = True,
                 range_: int = 0, index_base: int = 0, stream=None):
        """The k best entries the latest push completed on every listed channel: window_device, then
        Corpus.query_packed_recording_topk_tail_batch_keys_device on its output, on ONE stream with nothing in between.
        new_counts as new_occurrences takes them.  Returns (keys int64 [len(channels), k], lags int32 of the same shape) -- the
        keys alone with aligned=False --: per channel the entries whose best NEW cell scores above 0, best first, zeros behind
        them; an entry is reported at most once per push.  Decode with decode_tail_matches and totals()."""
        if not hasattr(new_counts, "data_ptr"):
            ch, _ = _u32_list(channels)
            new_counts = np.asarray(new_counts).reshape(-1)[ch]
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_recording_topk_tail_batch_keys_device(packed, packed.shape[0], n, new_counts, k, max_new=max_new,
                                                                         range_=range_, index_base=index_base, aligned=aligned,
                                                                         stream=stream)

    def new_matches_above(self, corpus: "Corpus", channels, n: int, new_counts, threshold: float, capacity: int, max_new: int = None,
                          range_: int = 0, index_base: int = 0, want_lags: bool = True, stream=None):
        """Every entry the latest push completed at or above `threshold` on every listed channel: window_device, then
        Corpus.query_packed_recording_threshold_tail_batch_keys_device on its output, on ONE stream with nothing in between.
        new_counts as new_occurrences takes them.  Returns (keys int64 [len(channels), capacity], lags int32 of the same shape or
        None, counts int64 [len(channels)]): per channel the distinct entries of new_occurrences' row in ascending index, each
        once with its best new cell.  Decode with decode_tail_matches and totals()."""
        if not hasattr(new_counts, "data_ptr"):
            ch, _ = _u32_list(channels)
            new_counts = np.asarray(new_counts).reshape(-1)[ch]
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_recording_threshold_tail_batch_keys_device(packed, packed.shape[0], n, new_counts, threshold, capacity,
                                                                              max_new=max_new, range_=range_, index_base=index_base,
                                                                              want_lags=want_lags, stream=stream)

    def matches_above(self, corpus: "Corpus", channels, n: int, threshold: float, capacity: int, range_: int = 0, index_base: int = 0,
                      want_lags: bool = True, stream=None):
        """Every entry the window of every listed channel matches at or above `threshold`: window_device, then
        Corpus.query_packed_recording_threshold_batch_keys_device on its output, on ONE stream with nothing in between.  Returns
        (keys int64 [len(channels), capacity], lags int32 of the same shape or None, counts int64 [len(channels)]): per channel
        the entries in ascending index with the lag of their best cell."""
        packed = self.window_device(channels, n, stream=stream)
        return corpus.query_packed_recording_threshold_batch_keys_device(packed, packed.shape[0], n, threshold, capacity, range_=range_,
                                                                         index_base=index_base, want_lags=want_lags, stream=stream)

def debug_resampler_bank_plan(rate_in: float, rate_out: float, mode: int, input_totals, output_totals, counts, finish: bool = False):
    """LBAudioDetectiveDebugResamplerBankPlan (tests): the host plan of one resampler-bank call -> (new, carried, m_lo, m_hi): the
    samples every channel emits and carries afterwards (uint32 arrays, one value per channel) and the rate pair's tap range.
    Needs no GPU."""
    li = np.ascontiguousarray(np.asarray(input_totals).reshape(-1), dtype=np.uint64)
    lo = np.ascontiguousarray(np.asarray(output_totals).reshape(-1), dtype=np.uint64)
    n, npt = _u32_list(counts)
    if not li.size == lo.size == n.size:
        raise ValueError("input totals, output totals and counts must have one value per channel")
    out = [np.zeros(max(1, n.size), np.uint32) for _ in range(2)]
    taps = [N.SInt32(0), N.SInt32(0)]
    u64p = C.POINTER(N.UInt64)
    _check(N.lib().LBAudioDetectiveDebugResamplerBankPlan(rate_in, rate_out, mode, n.size, li.ctypes.data_as(u64p) if li.size else None,
                                                          lo.ctypes.data_as(u64p) if lo.size else None, npt, 1 if finish else 0,
                                                          *[o.ctypes.data_as(C.POINTER(N.UInt32)) for o in out],
                                                          *[C.byref(t) for t in taps]), "DebugResamplerBankPlan")
    return out[0][:n.size], out[1][:n.size], int(taps[0].value), int(taps[1].value)


class ResamplerBank:
    """LBAudioDetectiveResamplerBankRef: `channels` live channels converted from `rate_in` to `rate_out` on the device, their filter
    history kept there between pushes.  A push takes new samples (float32 or int16) of any of the channels and emits every output
    sample that became final, laid out as StreamBank.push_device takes them; `feed` runs both pushes on one stream.  After L samples
    in any chunking a channel has emitted a prefix of what the whole-signal converter gives, bit for bit; `finish` emits the rest."""

    def __init__(self, rate_in: float, rate_out: float, channels: int, mode: int = 0):
        self._L = N.lib()
        self.rate_in, self.rate_out, self.n_channels, self.mode = float(rate_in), float(rate_out), int(channels), int(mode)
        self._ref = self._L.LBAudioDetectiveResamplerBankNew(self.rate_in, self.rate_out, self.mode, self.n_channels)
        if not self._ref:
            raise LBAudioDetectiveError(1, "ResamplerBankNew (equal or unsupported rates, mode above 1, zero channels or no HIP device)")

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveResamplerBankDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def _plan_total(self, counts, finish=False) -> int:
        li, lo = self.totals()
        return int(debug_resampler_bank_plan(self.rate_in, self.rate_out, self.mode, li, lo, counts, finish)[0].sum(dtype=np.uint64))

    def _out(self, out, total, stream):
        import torch
        if out is None:                      # sized from the plan, which the host can make alone
            with torch.cuda.stream(stream):  # (the block belongs to the stream that fills it)
                out = torch.empty(total, dtype=torch.float32, device="cuda")
        if not out.is_cuda or not out.is_contiguous() or out.dtype != torch.float32:
            raise ValueError("out must be a contiguous float32 device tensor")
        return out

    def _emit(self, call, what, out, stream):
        new_counts = np.zeros(self.n_channels, np.uint32)
        total = N.UInt64(0)
        _check(call(new_counts.ctypes.data_as(C.POINTER(N.UInt32)), _dev_ptr(out) if out.numel() else None, out.numel(), C.byref(total),
                    _stream_ptr(stream)), what)
        return new_counts, out.reshape(-1)[:total.value]

    def _push(self, fn, what, samples_ptr, fmt, counts, out, stream):
        n, npt = _u32_list(counts)
        if n.size != self.n_channels:
            raise ValueError("counts must have one value per channel")
        out = self._out(out, self._plan_total(n) if out is None else 0, stream)
        return self._emit(lambda *rest: fn(self._ref, samples_ptr, fmt, npt, *rest), what, out, stream)

    def push_device(self, samples, counts, out=None, stream=None):
        """LBAudioDetectiveResamplerBankPushDevice: `samples`, a float32 or int16 device tensor holding the channels' new samples one
        after the other in channel order; `counts`, one host integer per channel.  out: None (a tensor of exactly the emitted
        samples is made) or a contiguous float32 device tensor with room for them -> (new_counts uint32 [channels] on the host,
        the emitted samples float32 [total] on the device in channel order then time order).  Asynchronous on `stream`; `samples`
        must stay untouched until the stream has run the call."""
        import torch
        if not samples.is_cuda or not samples.is_contiguous() or samples.dtype not in (torch.float32, torch.int16):
            raise ValueError("samples must be a contiguous float32 or int16 device tensor")
        if samples.numel() < int(np.asarray(counts, dtype=np.uint64).sum()):
            raise ValueError("samples holds fewer values than the counts add up to")
        return self._push(self._L.LBAudioDetectiveResamplerBankPushDevice, "ResamplerBankPushDevice",
                          C.c_void_p(samples.data_ptr()) if samples.numel() else None, 1 if samples.dtype == torch.int16 else 0, counts, out,
                          stream)

    def push(self, chunks, out=None, stream=None):
        """LBAudioDetectiveResamplerBankPush: `chunks`, one numpy array of new samples per channel (None or empty: nothing for that
        channel), from host memory -- int16 when every array given is int16, float32 when none is, ValueError for a mixture;
        returns as push_device once the samples have been taken."""
        if len(chunks) != self.n_channels:
            raise ValueError("chunks must have one entry per channel")
        given = [np.asarray(c) for c in chunks if c is not None and np.asarray(c).size]
        as_int = [g.dtype == np.int16 for g in given]
        if any(as_int) and not all(as_int):      # (an int16 sample is s / 32768, not s: one push has one format)
            raise ValueError("chunks mix int16 arrays with others: one push has one sample format")
        dtype = np.int16 if given and all(as_int) else np.float32
        parts = [np.ascontiguousarray(c, dtype=dtype).reshape(-1) if c is not None else np.zeros(0, dtype) for c in chunks]
        x = np.concatenate(parts) if parts else np.zeros(0, dtype)
        return self._push(self._L.LBAudioDetectiveResamplerBankPush, "ResamplerBankPush", C.c_void_p(x.ctypes.data) if x.size else None,
                          1 if dtype == np.int16 else 0, [p.size for p in parts], out, stream)

    def finish(self, channels, out=None, stream=None):
        """LBAudioDetectiveResamplerBankFinishChannels: the listed channels end their signals where they are -> (new_counts, the
        samples the whole-signal converter still has for them, in channel order), and start again."""
        ch, cp = _u32_list(channels)
        if out is None:
            listed = np.zeros(self.n_channels, bool)
            listed[ch[ch < self.n_channels]] = True
            li, lo = self.totals()
            new = debug_resampler_bank_plan(self.rate_in, self.rate_out, self.mode, li, lo, np.zeros(self.n_channels, np.uint32), True)[0]
            out = self._out(None, int(new[listed].sum(dtype=np.uint64)), stream)
        else:
            out = self._out(out, 0, stream)
        return self._emit(lambda *rest: self._L.LBAudioDetectiveResamplerBankFinishChannels(self._ref, cp, ch.size, *rest),
                          "ResamplerBankFinishChannels", out, stream)

    def totals(self):
        """(samples received, samples emitted) of every channel since it (re)started (uint64 arrays, the host mirror)"""
        out = [np.zeros(self.n_channels, np.uint64) for _ in range(2)]
        _check(self._L.LBAudioDetectiveResamplerBankGetCounts(self._ref, *[o.ctypes.data_as(C.POINTER(N.UInt64)) for o in out]),
               "ResamplerBankGetCounts")
        return out[0], out[1]

    def reset(self, channels):
        """LBAudioDetectiveResamplerBankResetChannels: the listed channels start again, emitting nothing."""
        ch, cp = _u32_list(channels)
        _check(self._L.LBAudioDetectiveResamplerBankResetChannels(self._ref, cp, ch.size), "ResamplerBankResetChannels")

    def feed(self, stream_bank: "StreamBank", samples, counts, new_out=None, stream=None):
        """The live path: push_device, then stream_bank.push_device on what it emitted, on ONE stream with nothing read back.
        Returns what StreamBank.push_device returns."""
        new_counts, converted = self.push_device(samples, counts, stream=stream)
        return stream_bank.push_device(converted, new_counts, new_out=new_out, stream=stream)


class Corpus:
    """LBAudioDetectiveCorpusRef: device-resident reference fingerprints with a top-1 query."""

    def __init__(self, subfingerprint_length: int, subfingerprints_per_entry: int, capacity: int, _ref=None):
        self._L = N.lib()
        self._ref = _ref if _ref is not None else self._L.LBAudioDetectiveCorpusNew(
            subfingerprint_length, subfingerprints_per_entry, capacity)
        if not self._ref:
            raise LBAudioDetectiveError(1, "CorpusNew (unsupported shape, zero capacity or no HIP device)")
        self.subfingerprint_length = subfingerprint_length
        self.subfingerprints_per_entry = subfingerprints_per_entry
        self.capacity = capacity

    @classmethod
    def ragged(cls, subfingerprint_length: int, entry_capacity: int, subfingerprint_capacity: int) -> "Corpus":
        """LBAudioDetectiveCorpusNewRagged: entries of any length (the shape of LBAudioDetectiveTests.m:57-91)."""
        ref = N.lib().LBAudioDetectiveCorpusNewRagged(subfingerprint_length, entry_capacity, subfingerprint_capacity)
        if not ref:
            raise LBAudioDetectiveError(1, "CorpusNewRagged (unsupported length, zero capacity or no HIP device)")
        return cls(subfingerprint_length, 0, entry_capacity, _ref=ref)

    def set_bound_pruning(self, enabled: bool):
        """Ragged corpora, top-1 queries: drop groups of sliding offsets that cannot reach the best match found so far
        (exact; on by default).  LBAudioDetectiveCorpusSetBoundPruning."""
        _check(self._L.LBAudioDetectiveCorpusSetBoundPruning(self._ref, 1 if enabled else 0), "CorpusSetBoundPruning")
        return self

    def set_bound_pruning_threshold(self, score: float):
        """The score from which a match is published and bounds the rest of a top-1 scan (default 0.7)."""
        _check(self._L.LBAudioDetectiveCorpusSetBoundPruningThreshold(self._ref, float(score)), "CorpusSetBoundPruningThreshold")
        return self

    @property
    def bound_pruning_threshold(self) -> float:
        return float(self._L.LBAudioDetectiveCorpusGetBoundPruningThreshold(self._ref))

    @property
    def subfingerprint_total(self) -> int:
        return int(self._L.LBAudioDetectiveCorpusGetSubfingerprintTotal(self._ref))

    def append_ragged_packed_device(self, packed, counts, stream=None):
        """packed: torch uint8 [sum(counts), 32] on the device; counts: the entries' sub-fingerprint counts (host)."""
        assert packed.is_cuda and packed.is_contiguous()
        cnt = np.ascontiguousarray(counts, dtype=np.uint32)
        assert int(cnt.sum()) == packed.shape[0]
        _check(self._L.LBAudioDetectiveCorpusAppendRaggedPackedDevice(self._ref, packed.data_ptr(), cnt.ctypes.data,
                                                                     cnt.size, _stream_ptr(stream)),
               "CorpusAppendRaggedPackedDevice")

    def dispose(self):
        if self._ref:
            self._L.LBAudioDetectiveCorpusDispose(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._L.LBAudioDetectiveCorpusGetCount(self._ref))

    def save(self, path: str):
        _check(self._L.LBAudioDetectiveCorpusSave(self._ref, path.encode()), "CorpusSave")

    @classmethod
    def load(cls, path: str, subfingerprint_length: int, subfingerprints_per_entry: int, capacity: int = 0) -> "Corpus":
        ref = N.lib().LBAudioDetectiveCorpusLoad(path.encode(), capacity)
        if not ref:
            raise LBAudioDetectiveError(1, "CorpusLoad (missing/malformed file or no HIP device)")
        c = cls(subfingerprint_length, subfingerprints_per_entry, capacity, _ref=ref)
        return c

    @property
    def entry_stride_bytes(self) -> int:
        return int(self._L.LBAudioDetectiveCorpusGetEntryStrideBytes(self._ref))

    def set_kernel_variant(self, variant: int):
        _check(self._L.LBAudioDetectiveCorpusSetKernelVariant(self._ref, variant), "CorpusSetKernelVariant")

    def append_packed_device(self, packed, stream=None):
        """packed: torch uint8 [n, per_entry, 32] on the device."""
        assert packed.is_cuda and packed.is_contiguous()
        n = packed.shape[0]
        _check(self._L.LBAudioDetectiveCorpusAppendPackedDevice(self._ref, packed.data_ptr(), n, _stream_ptr(stream)),
               "CorpusAppendPackedDevice")

    def append_fingerprint(self, fp: Fingerprint):
        _check(self._L.LBAudioDetectiveCorpusAppendFingerprint(self._ref, fp._ref), "CorpusAppendFingerprint")

    def query(self, fp: Fingerprint, range_: int = 0):
        idx, score = N.SInt64(-1), N.Float32(0.0)
        _check(self._L.LBAudioDetectiveCorpusQuery(self._ref, fp._ref, range_, C.byref(idx), C.byref(score)), "CorpusQuery")
        return int(idx.value), float(score.value)

    def query_batch(self, fps, range_: int = 0):
        """Several queries in one pass over the corpus -> list of (index, score)."""
        n = len(fps)
        refs = (N.Ref * n)(*[f._ref for f in fps])
        idx, sc = (N.SInt64 * n)(), (N.Float32 * n)()
        _check(self._L.LBAudioDetectiveCorpusQueryBatch(self._ref, refs, n, range_, idx, sc), "CorpusQueryBatch")
        return [(int(idx[i]), float(sc[i])) for i in range(n)]

    def query_batch_keys_device(self, fps, keys_out, range_: int = 0, index_base: int = 0, stream=None):
        """Writes len(fps) 64-bit keys into keys_out (torch int64 on the device), asynchronously."""
        n = len(fps)
        refs = (N.Ref * n)(*[f._ref for f in fps])
        _check(self._L.LBAudioDetectiveCorpusQueryBatchKeysDevice(self._ref, refs, n, range_, index_base,
                                                                 keys_out.data_ptr(), _stream_ptr(stream)),
               "CorpusQueryBatchKeysDevice")
        return keys_out

    def query_key_device(self, fp: Fingerprint, key_out, range_: int = 0, index_base: int = 0, stream=None):
        """Writes the 64-bit (score, ~index) key into key_out (torch int64[1] on the device), async."""
        _check(self._L.LBAudioDetectiveCorpusQueryKeyDevice(self._ref, fp._ref, range_, index_base, key_out.data_ptr(),
                                                           _stream_ptr(stream)), "CorpusQueryKeyDevice")
        return key_out

    def query_sharded(self, fp: Fingerprint, comm: "Comm", index_base: int = 0, range_: int = 0, stream=None):
        """LBAudioDetectiveCorpusQuerySharded: this rank's scan + the library's own RCCL all-reduce (ncclUint64,
        ncclMax) of the key; collective, every rank gets (global index, score)."""
        idx, score = N.SInt64(-1), N.Float32(0.0)
        _check(self._L.LBAudioDetectiveCorpusQuerySharded(self._ref, fp._ref, range_, index_base, comm._ref,
                                                         _stream_ptr(stream), C.byref(idx), C.byref(score)),
               "CorpusQuerySharded")
        return int(idx.value), float(score.value)

    def query_batch_sharded(self, fps, comm: "Comm", index_base: int = 0, range_: int = 0, stream=None):
        n = len(fps)
        refs = (N.Ref * n)(*[f._ref for f in fps])
        idx, sc = (N.SInt64 * n)(), (N.Float32 * n)()
        _check(self._L.LBAudioDetectiveCorpusQueryBatchSharded(self._ref, refs, n, range_, index_base, comm._ref,
                                                              _stream_ptr(stream), idx, sc), "CorpusQueryBatchSharded")
        return [(int(idx[i]), float(sc[i])) for i in range(n)]

    def query_batch_sharded_with(self, fps, all_reduce, index_base: int = 0, range_: int = 0, stream=None, context=None):
        """LBAudioDetectiveCorpusQueryBatchShardedWith: the sharded query with the caller's exchange step --
        all_reduce(context, device_keys_ptr, count, stream_ptr) -> status must leave the element-wise MAX over all
        ranks in the `count` unsigned 64-bit keys at device_keys_ptr.  `self` may be None-like (pass corpus=None through
        sharded_query_without_corpus) only from tests of the failing-rank path."""
        n = len(fps)
        refs = (N.Ref * n)(*[f._ref for f in fps])
        idx, sc = (N.SInt64 * n)(), (N.Float32 * n)()
        cb = all_reduce if isinstance(all_reduce, N.AllReduceMaxFn) else N.AllReduceMaxFn(all_reduce)
        st = self._L.LBAudioDetectiveCorpusQueryBatchShardedWith(self._ref, refs, n, range_, index_base, cb, context,
                                                                _stream_ptr(stream), idx, sc)
        _check(st, "CorpusQueryBatchShardedWith")
        return [(int(idx[i]), float(sc[i])) for i in range(n)]

    def scores_device(self, fp: Fingerprint, range_: int = 0, stream=None):
        import torch
        out = torch.empty(len(self), dtype=torch.float32, device="cuda")
        _check(self._L.LBAudioDetectiveCorpusScoresDevice(self._ref, fp._ref, range_, out.data_ptr(), _stream_ptr(stream)),
               "CorpusScoresDevice")
        return out

    def query_topk(self, fp: Fingerprint, k: int, range_: int = 0):
        """The k best matches (LBAudioDetectiveCorpusQueryTopK): (indices int64[n], scores float32[n]), score descending,
        equal scores lowest index first, n = min(k, entries scoring above 0); k = 1 is query()'s answer."""
        return self.query_batch_topk([fp], k, range_)[0]

    def query_batch_topk(self, fps, k: int, range_: int = 0):
        """query_topk for several queries in one call -> list of (indices, scores); equal to separate calls, bit for bit."""
        n = len(fps)
        refs = (N.Ref * max(1, n))(*[f._ref for f in fps])
        idx = np.full((max(1, n), max(1, k)), -1, dtype=np.int64)
        sc = np.zeros((max(1, n), max(1, k)), dtype=np.float32)
        cnt = np.zeros(max(1, n), dtype=np.uint32)
        _check(self._L.LBAudioDetectiveCorpusQueryBatchTopK(self._ref, refs, n, range_, k, idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                            sc.ctypes.data_as(C.POINTER(N.Float32)),
                                                            cnt.ctypes.data_as(C.POINTER(N.UInt32))), "CorpusQueryBatchTopK")
        return [(idx[i, :cnt[i]].copy(), sc[i, :cnt[i]].copy()) for i in range(n)]

    def query_batch_topk_keys_device(self, fps, k: int, keys_out, range_: int = 0, index_base: int = 0, stream=None):
        """Writes len(fps) x k 64-bit keys (global index = index_base + local; rows descending, 0-padded) into keys_out
        (torch int64 on the device, contiguous), asynchronously."""
        n = len(fps)
        if keys_out.numel() < n * k or not keys_out.is_contiguous():
            raise ValueError("keys_out must be a contiguous tensor of at least len(fps) * k int64")
        refs = (N.Ref * max(1, n))(*[f._ref for f in fps])
        _check(self._L.LBAudioDetectiveCorpusQueryBatchTopKKeysDevice(self._ref, refs, n, range_, k, index_base,
                                                                     keys_out.data_ptr(), _stream_ptr(stream)),
               "CorpusQueryBatchTopKKeysDevice")
        return keys_out

    # ---- packed queries: fingerprints already on the device (what Detective.fingerprint_clips_device writes), no handles and
    # no host round trip.  `packed`: a torch tensor on the device (uint8 [n, per, 32], or anything contiguous of that size) or
    # a raw device address; the outputs likewise (a raw address is returned as given).
    def query_packed_keys_device(self, packed, n_queries: int, per_query: int, keys_out=None, range_: int = 0, index_base: int = 0,
                                 stream=None):
        """LBAudioDetectiveCorpusQueryPackedKeysDevice: n_queries 64-bit keys (torch int64 on the device), equal to
        query_batch_keys_device's for fingerprints with the same Booleans; asynchronous on `stream`."""
        _packed_ok(packed, n_queries, per_query)
        if keys_out is None:
            import torch
            keys_out = torch.empty(max(1, n_queries), dtype=torch.int64, device=packed.device if hasattr(packed, "device") else "cuda")
        _out_ok(keys_out, n_queries, "keys_out")
        _check(self._L.LBAudioDetectiveCorpusQueryPackedKeysDevice(self._ref, _dev_ptr(packed), n_queries, per_query, range_, index_base,
                                                                  _dev_ptr(keys_out), _stream_ptr(stream)), "CorpusQueryPackedKeysDevice")
        return keys_out

    def query_packed_topk_keys_device(self, packed, n_queries: int, per_query: int, k: int, keys_out=None, lags_out=None,
                                      aligned: bool = False, range_: int = 0, index_base: int = 0, stream=None):
        """LBAudioDetectiveCorpusQueryPackedTopKKeysDevice: n_queries x k keys (torch int64 [n, k] on the device, rows descending,
        0-padded), equal to query_batch_topk_keys_device's; with aligned=True (or a lags_out) also the n x k int32 lags
        align_keys_device gives for those keys -> (keys, lags).  Asynchronous on `stream`."""
        _packed_ok(packed, n_queries, per_query)
        want_lags = aligned or lags_out is not None
        if keys_out is None or (want_lags and lags_out is None):
            import torch
            dev = packed.device if hasattr(packed, "device") else "cuda"
            if keys_out is None:
                keys_out = torch.empty((max(1, n_queries), max(1, k)), dtype=torch.int64, device=dev)
            if want_lags and lags_out is None:
                lags_out = torch.empty((max(1, n_queries), max(1, k)), dtype=torch.int32, device=dev)
        _out_ok(keys_out, n_queries * k, "keys_out")
        if want_lags:
            _out_ok(lags_out, n_queries * k, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusQueryPackedTopKKeysDevice(self._ref, _dev_ptr(packed), n_queries, per_query, range_, k,
                                                                      index_base, _dev_ptr(keys_out),
                                                                      _dev_ptr(lags_out) if want_lags else None,
                                                                      _stream_ptr(stream)), "CorpusQueryPackedTopKKeysDevice")
        return (keys_out, lags_out) if want_lags else keys_out

    # ---- threshold queries: every entry whose score is >= threshold (a float32 compare), in ascending entry index, the first
    # `capacity` of them; the count is always the true number of matches (count > capacity: the list was cut)
    def query_threshold(self, fp: Fingerprint, threshold: float, capacity: int, range_: int = 0, aligned: bool = False):
        """LBAudioDetectiveCorpusQueryThreshold: (indices int64[m], scores float32[m], count) with m = min(count, capacity), or
        with aligned=True (indices, scores, lags int32[m], count)."""
        return self.query_threshold_batch([fp], threshold, capacity, range_, aligned)[0]

    def query_threshold_batch(self, fps, threshold: float, capacity: int, range_: int = 0, aligned: bool = False):
        """query_threshold for several queries in one call -> list of its tuples; equal to separate calls, bit for bit."""
        n = len(fps)
        refs = (N.Ref * max(1, n))(*[f._ref for f in fps])
        shape = (max(1, n), max(1, capacity))
        idx = np.full(shape, -1, dtype=np.int64)
        sc = np.zeros(shape, dtype=np.float32)
        lag = np.zeros(shape if aligned else (1, 1), dtype=np.int32)
        cnt = np.zeros(max(1, n), dtype=np.uint64)
        pi, ps = idx.ctypes.data_as(C.POINTER(N.SInt64)), sc.ctypes.data_as(C.POINTER(N.Float32))
        pc = cnt.ctypes.data_as(C.POINTER(N.UInt64))
        if aligned:
            _check(self._L.LBAudioDetectiveCorpusQueryBatchThresholdAligned(self._ref, refs, n, range_, threshold, capacity, pi, ps,
                                                                            lag.ctypes.data_as(C.POINTER(N.SInt32)), pc),
                   "CorpusQueryBatchThresholdAligned")
        else:
            _check(self._L.LBAudioDetectiveCorpusQueryBatchThreshold(self._ref, refs, n, range_, threshold, capacity, pi, ps, pc),
                   "CorpusQueryBatchThreshold")
        out = []
        for i in range(n):
            m = min(int(cnt[i]), capacity)
            out.append((idx[i, :m].copy(), sc[i, :m].copy()) + ((lag[i, :m].copy(),) if aligned else ()) + (int(cnt[i]),))
        return out

    def query_batch_threshold_keys_device(self, fps, threshold: float, capacity: int, keys_out=None, counts_out=None, range_: int = 0,
                                          index_base: int = 0, stream=None):
        """LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice: (keys int64 [len(fps), capacity], counts int64 [len(fps)]) on the
        device (global index = index_base + local; rows in ascending index, 0-padded; decode a row with decode_threshold_keys),
        asynchronously on `stream`."""
        n = len(fps)
        keys_out, counts_out, _ = _threshold_out(n, capacity, keys_out, counts_out, None, False, "cuda")
        refs = (N.Ref * max(1, n))(*[f._ref for f in fps])
        _check(self._L.LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(self._ref, refs, n, range_, threshold, capacity, index_base,
                                                                          _dev_ptr(keys_out), _dev_ptr(counts_out),
                                                                          _stream_ptr(stream)), "CorpusQueryBatchThresholdKeysDevice")
        return keys_out, counts_out

    def query_packed_threshold_keys_device(self, packed, n_queries: int, per_query: int, threshold: float, capacity: int,
                                           keys_out=None, counts_out=None, lags_out=None, aligned: bool = False, range_: int = 0,
                                           index_base: int = 0, stream=None):
        """LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice: query_batch_threshold_keys_device's (keys, counts) for packed
        fingerprints already on the device; with aligned=True (or a lags_out) also the int32 lags [n, capacity] -> (keys, counts,
        lags).  Asynchronous on `stream`, nothing visits the host."""
        _packed_ok(packed, n_queries, per_query)
        want_lags = aligned or lags_out is not None
        dev = packed.device if hasattr(packed, "device") else "cuda"
        keys_out, counts_out, lags_out = _threshold_out(n_queries, capacity, keys_out, counts_out, lags_out, want_lags, dev)
        _check(self._L.LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice(self._ref, _dev_ptr(packed), n_queries, per_query, range_,
                                                                           threshold, capacity, index_base, _dev_ptr(keys_out),
                                                                           _dev_ptr(counts_out),
                                                                           _dev_ptr(lags_out) if want_lags else None,
                                                                           _stream_ptr(stream)), "CorpusQueryPackedThresholdKeysDevice")
        return (keys_out, counts_out, lags_out) if want_lags else (keys_out, counts_out)

    # ---- corpus join: the entries of a corpus (this one, or `queries`) as queries against this corpus -- every ORDERED pair
    # (row, entry) whose score is >= threshold, rows ascending, entries ascending inside a row, as CSR.  Uniform corpora of one
    # shape (sub-fingerprints of 200 Booleans, 1 .. 8 per entry).
    def _join_args(self, queries, first, count, skip_same_index):
        q = self if queries is None else queries
        if count is None:
            count = len(q) - first
        if skip_same_index is None:
            skip_same_index = q is self
        return q, int(first), int(count), int(bool(skip_same_index))

    def join_threshold_keys_device(self, threshold: float, capacity: int, queries=None, first: int = 0, count=None,
                                   skip_same_index=None, range_: int = 0, index_base: int = 0, keys_out=None, offsets_out=None,
                                   stream=None):
        """LBAudioDetectiveCorpusJoinThresholdKeysDevice: (keys int64 [capacity], offsets int64 [count + 1]) on the device,
        asynchronously on `stream`.  The rows are entries first .. first + count - 1 of `queries` (None: this corpus, a
        self-join); offsets[r] = matches of the rows before r, offsets[count] = the true total (above the capacity: the list
        was cut); slot p holds the p-th match's key (global entry index = index_base + local), zero keys behind the matches.
        skip_same_index (None: on for a self-join, off otherwise) leaves out the pair whose row index equals the entry's index.
        Decode with decode_join_keys."""
        q, first, count, skip = self._join_args(queries, first, count, skip_same_index)
        if keys_out is None or offsets_out is None:
            import torch
            if keys_out is None:
                keys_out = torch.empty(max(1, capacity), dtype=torch.int64, device="cuda")
            if offsets_out is None:
                offsets_out = torch.empty(max(1, count) + 1, dtype=torch.int64, device="cuda")
        _out_ok(keys_out, capacity, "keys_out")
        _out_ok(offsets_out, count + 1, "offsets_out")
        _check(self._L.LBAudioDetectiveCorpusJoinThresholdKeysDevice(self._ref, q._ref, first, count, range_, threshold, skip, capacity,
                                                                    index_base, _dev_ptr(keys_out), _dev_ptr(offsets_out),
                                                                    _stream_ptr(stream)), "CorpusJoinThresholdKeysDevice")
        return keys_out, offsets_out

    def join_threshold(self, threshold: float, capacity: int, queries=None, first: int = 0, count=None, skip_same_index=None,
                       range_: int = 0):
        """LBAudioDetectiveCorpusJoinThreshold: (rows int64[m], indices int64[m], scores float32[m], total) with m = min(total,
        capacity): the pairs (row index in `queries`, entry index, score) in the device form's order."""
        q, first, count, skip = self._join_args(queries, first, count, skip_same_index)
        rows = np.full(max(1, capacity), -1, dtype=np.int64)
        idx = np.full(max(1, capacity), -1, dtype=np.int64)
        sc = np.zeros(max(1, capacity), dtype=np.float32)
        total = N.UInt64(0)
        _check(self._L.LBAudioDetectiveCorpusJoinThreshold(self._ref, q._ref, first, count, range_, threshold, skip, capacity,
                                                          rows.ctypes.data_as(C.POINTER(N.SInt64)),
                                                          idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                          sc.ctypes.data_as(C.POINTER(N.Float32)), C.byref(total)), "CorpusJoinThreshold")
        m = min(int(total.value), capacity)
        return rows[:m].copy(), idx[:m].copy(), sc[:m].copy(), int(total.value)

    # ---- the join of RAGGED corpora (Corpus.ragged): the same CSR; the score is the ragged scan's (the shorter entry slides along
    # the longer) and every match comes with its signed lag.  No entry of either corpus above LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS (the header).
    def join_ragged_threshold_keys_device(self, threshold: float, capacity: int, queries=None, first: int = 0, count=None,
                                          skip_same_index=None, range_: int = 0, index_base: int = 0, keys_out=None, lags_out=None,
                                          offsets_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusJoinRaggedThresholdKeysDevice: (keys int64 [capacity], lags int32 [capacity] or None, offsets
        int64 [count + 1]) on the device, asynchronously on `stream`; join_threshold_keys_device's arguments and layout.
        lags[p] is the lag of the match in slot p (+offset: the entry is longer than the row; -offset otherwise; 0 behind the
        matches), what align_keys_device gives for that row and key.  want_lags=False (and no lags_out) passes NULL: the keys
        and offsets are the same."""
        q, first, count, skip = self._join_args(queries, first, count, skip_same_index)
        import torch
        if keys_out is None:
            keys_out = torch.empty(max(1, capacity), dtype=torch.int64, device="cuda")
        if lags_out is None and want_lags:
            lags_out = torch.empty(max(1, capacity), dtype=torch.int32, device="cuda")
        if offsets_out is None:
            offsets_out = torch.empty(max(1, count) + 1, dtype=torch.int64, device="cuda")
        _out_ok(keys_out, capacity, "keys_out")
        _out_ok(offsets_out, count + 1, "offsets_out")
        if lags_out is not None:
            _out_ok(lags_out, capacity, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusJoinRaggedThresholdKeysDevice(
            self._ref, q._ref, first, count, range_, threshold, skip, capacity, index_base, _dev_ptr(keys_out),
            _dev_ptr(lags_out) if lags_out is not None else None, _dev_ptr(offsets_out), _stream_ptr(stream)),
            "CorpusJoinRaggedThresholdKeysDevice")
        return keys_out, lags_out, offsets_out

    def join_ragged_threshold(self, threshold: float, capacity: int, queries=None, first: int = 0, count=None, skip_same_index=None,
                              range_: int = 0):
        """LBAudioDetectiveCorpusJoinRaggedThreshold: (rows int64[m], indices int64[m], scores float32[m], lags int32[m], total)
        with m = min(total, capacity), in the device form's order."""
        q, first, count, skip = self._join_args(queries, first, count, skip_same_index)
        rows = np.full(max(1, capacity), -1, dtype=np.int64)
        idx = np.full(max(1, capacity), -1, dtype=np.int64)
        sc = np.zeros(max(1, capacity), dtype=np.float32)
        lags = np.zeros(max(1, capacity), dtype=np.int32)
        total = N.UInt64(0)
        _check(self._L.LBAudioDetectiveCorpusJoinRaggedThreshold(self._ref, q._ref, first, count, range_, threshold, skip, capacity,
                                                                rows.ctypes.data_as(C.POINTER(N.SInt64)),
                                                                idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                                sc.ctypes.data_as(C.POINTER(N.Float32)),
                                                                lags.ctypes.data_as(C.POINTER(N.SInt32)), C.byref(total)),
               "CorpusJoinRaggedThreshold")
        m = min(int(total.value), capacity)
        return rows[:m].copy(), idx[:m].copy(), sc[:m].copy(), lags[:m].copy(), int(total.value)

    # ---- occurrences: every place ONE query (a long recording) matches a ragged corpus -- each cell (entry, sliding offset) of
    # match_profile's values that is >= threshold, with peaks=True only the local peaks of every profile; entries ascending,
    # offsets ascending inside an entry.  The total is always the true number of matching cells.
    def query_occurrences(self, fp: Fingerprint, threshold: float, capacity: int, peaks: bool = False, range_: int = 0):
        """LBAudioDetectiveCorpusQueryOccurrences: (indices int64[m], scores float32[m], lags int32[m], total) with m = min(total,
        capacity).  lags[p] is +offset when the entry is longer than the query, -offset otherwise."""
        idx = np.full(max(1, capacity), -1, dtype=np.int64)
        sc = np.zeros(max(1, capacity), dtype=np.float32)
        lags = np.zeros(max(1, capacity), dtype=np.int32)
        total = N.UInt64(0)
        _check(self._L.LBAudioDetectiveCorpusQueryOccurrences(self._ref, fp._ref, range_, threshold, int(bool(peaks)), capacity,
                                                             idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                             sc.ctypes.data_as(C.POINTER(N.Float32)),
                                                             lags.ctypes.data_as(C.POINTER(N.SInt32)), C.byref(total)),
               "CorpusQueryOccurrences")
        m = min(int(total.value), capacity)
        return idx[:m].copy(), sc[:m].copy(), lags[:m].copy(), int(total.value)

    def query_occurrences_keys_device(self, fp: Fingerprint, threshold: float, capacity: int, peaks: bool = False, range_: int = 0,
                                      index_base: int = 0, keys_out=None, lags_out=None, count_out=None, want_lags: bool = True,
                                      stream=None):
        """LBAudioDetectiveCorpusQueryOccurrencesKeysDevice: (keys int64 [capacity], lags int32 [capacity] or None, count int64
        [1]) on the device, asynchronously on `stream`; slot p holds match p (global entry index = index_base + local), zero keys
        and lags behind min(count, capacity).  want_lags=False (and no lags_out) passes NULL: keys and count are the same.
        Decode with decode_occurrence_keys."""
        keys_out, lags_out, count_out = _occurrences_out(capacity, keys_out, lags_out, count_out, want_lags, "cuda")
        _check(self._L.LBAudioDetectiveCorpusQueryOccurrencesKeysDevice(
            self._ref, fp._ref, range_, threshold, int(bool(peaks)), capacity, index_base, _dev_ptr(keys_out),
            _dev_ptr(lags_out) if lags_out is not None else None, _dev_ptr(count_out), _stream_ptr(stream)),
            "CorpusQueryOccurrencesKeysDevice")
        return keys_out, lags_out, count_out

    def query_packed_occurrences_keys_device(self, packed, per_query: int, threshold: float, capacity: int, peaks: bool = False,
                                             range_: int = 0, index_base: int = 0, keys_out=None, lags_out=None, count_out=None,
                                             want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedOccurrencesKeysDevice: query_occurrences_keys_device's result for ONE query of
        per_query packed sub-fingerprints already on the device (what Detective.fingerprint_clips_device writes); nothing
        visits the host."""
        _packed_ok(packed, 1, per_query)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        keys_out, lags_out, count_out = _occurrences_out(capacity, keys_out, lags_out, count_out, want_lags, dev)
        _check(self._L.LBAudioDetectiveCorpusQueryPackedOccurrencesKeysDevice(
            self._ref, _dev_ptr(packed), per_query, range_, threshold, int(bool(peaks)), capacity, index_base, _dev_ptr(keys_out),
            _dev_ptr(lags_out) if lags_out is not None else None, _dev_ptr(count_out), _stream_ptr(stream)),
            "CorpusQueryPackedOccurrencesKeysDevice")
        return keys_out, lags_out, count_out

    # ---- recording scores: every entry's score and lag for ONE query of any length (a long recording above all) against a
    # ragged corpus, with the occurrences pass' pair loop (n_entry steps per pass); scores_device's scores and
    # align_keys_device's lags, bit for bit
    def recording_scores_device(self, fp: Fingerprint = None, packed=None, per_query: int = 0, range_: int = 0, scores_out=None,
                                lags_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusRecordingScoresDevice (fp) / ...RecordingPackedScoresDevice (packed: per_query packed
        sub-fingerprints already on the device): (scores float32 [len(self)], lags int32 [len(self)] or None) on the device,
        asynchronously on `stream`.  lags[j] is +offset when entry j is longer than the query, -offset otherwise: the lowest
        offset that reaches scores[j].  want_lags=False (and no lags_out) passes NULL: the scores are the same."""
        if (fp is None) == (packed is None):
            raise ValueError("give either fp or packed")
        dev = packed.device if hasattr(packed, "device") else "cuda"
        n = len(self)
        if scores_out is None or (want_lags and lags_out is None):
            import torch
            if scores_out is None:
                scores_out = torch.empty(max(1, n), dtype=torch.float32, device=dev)[:n]
            if want_lags and lags_out is None:
                lags_out = torch.empty(max(1, n), dtype=torch.int32, device=dev)[:n]
        _out_ok(scores_out, n, "scores_out")
        if lags_out is not None:
            _out_ok(lags_out, n, "lags_out")
        lp = _dev_ptr(lags_out) if lags_out is not None else None
        if fp is not None:
            _check(self._L.LBAudioDetectiveCorpusRecordingScoresDevice(self._ref, fp._ref, range_, _dev_ptr(scores_out), lp,
                                                                      _stream_ptr(stream)), "CorpusRecordingScoresDevice")
        else:
            _packed_ok(packed, 1, per_query)
            _check(self._L.LBAudioDetectiveCorpusRecordingPackedScoresDevice(self._ref, _dev_ptr(packed), per_query, range_,
                                                                            _dev_ptr(scores_out), lp, _stream_ptr(stream)),
                   "CorpusRecordingPackedScoresDevice")
        return scores_out, lags_out

    def query_recording_topk(self, fp: Fingerprint, k: int, range_: int = 0):
        """LBAudioDetectiveCorpusQueryRecordingTopK: (indices int64[n], scores float32[n], lags int32[n]) of the k best entries,
        query_topk's order, n = min(k, entries scoring above 0)."""
        idx = np.full(max(1, k), -1, dtype=np.int64)
        sc = np.zeros(max(1, k), dtype=np.float32)
        lags = np.zeros(max(1, k), dtype=np.int32)
        cnt = N.UInt32(0)
        _check(self._L.LBAudioDetectiveCorpusQueryRecordingTopK(self._ref, fp._ref, range_, k, idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                               sc.ctypes.data_as(C.POINTER(N.Float32)),
                                                               lags.ctypes.data_as(C.POINTER(N.SInt32)), C.byref(cnt)),
               "CorpusQueryRecordingTopK")
        return idx[:cnt.value].copy(), sc[:cnt.value].copy(), lags[:cnt.value].copy()

    def query_packed_recording_topk_keys_device(self, packed, per_query: int, k: int, range_: int = 0, index_base: int = 0,
                                                keys_out=None, lags_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedRecordingTopKKeysDevice: (keys int64 [k], lags int32 [k] or None) on the device for ONE
        query of per_query packed sub-fingerprints already on the device: query_packed_topk_keys_device's keys and aligned lags
        (descending, 0-padded; a zero key has lag 0).  Asynchronous on `stream`, nothing visits the host."""
        _packed_ok(packed, 1, per_query)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        if keys_out is None or (want_lags and lags_out is None):
            import torch
            if keys_out is None:
                keys_out = torch.empty(max(1, k), dtype=torch.int64, device=dev)
            if want_lags and lags_out is None:
                lags_out = torch.empty(max(1, k), dtype=torch.int32, device=dev)
        _out_ok(keys_out, k, "keys_out")
        if lags_out is not None:
            _out_ok(lags_out, k, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusQueryPackedRecordingTopKKeysDevice(
            self._ref, _dev_ptr(packed), per_query, range_, k, index_base, _dev_ptr(keys_out),
            _dev_ptr(lags_out) if lags_out is not None else None, _stream_ptr(stream)), "CorpusQueryPackedRecordingTopKKeysDevice")
        return keys_out, lags_out

    def recording_scores_batch_device(self, packed, n_recordings: int, per_query: int, range_: int = 0, scores_out=None, lags_out=None,
                                      want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice: recording_scores_device for n_recordings recordings of per_query
        packed sub-fingerprints each, already on the device as [n_recordings, per_query, 32] bytes (StreamBank.window_device's
        block) -> (scores float32 [n_recordings, len(self)], lags int32 of the same shape or None) on the device, asynchronously on
        `stream`.  Row r is what recording_scores_device gives for recording r alone, bit for bit.  want_lags=False (and no
        lags_out) passes NULL: the scores are the same."""
        R, per = int(n_recordings), int(per_query)
        _packed_ok(packed, R, per)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        count = len(self)
        n = R * count
        if scores_out is None or (want_lags and lags_out is None):
            import torch
            with torch.cuda.stream(stream):              # (the blocks belong to the stream that fills them)
                if scores_out is None:
                    scores_out = torch.empty(max(1, n), dtype=torch.float32, device=dev)[:n].reshape(R, count)
                if want_lags and lags_out is None:
                    lags_out = torch.empty(max(1, n), dtype=torch.int32, device=dev)[:n].reshape(R, count)
        _out_ok(scores_out, n, "scores_out")
        if lags_out is not None:
            _out_ok(lags_out, n, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice(
            self._ref, _dev_ptr(packed), R, per, range_, _dev_ptr(scores_out), _dev_ptr(lags_out) if lags_out is not None else None,
            _stream_ptr(stream)), "CorpusRecordingPackedScoresBatchDevice")
        return scores_out, lags_out

    def query_packed_recording_topk_batch_keys_device(self, packed, n_recordings: int, per_query: int, k: int, range_: int = 0,
                                                      index_base: int = 0, keys_out=None, lags_out=None, aligned: bool = False,
                                                      stream=None):
        """LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice: the k best entries of n_recordings recordings of per_query
        packed sub-fingerprints each, already on the device as [n_recordings, per_query, 32] bytes -> the [n_recordings, k] int64
        key tensor (rows descending, 0-padded), and with aligned=True (or a lags_out) (keys, lags int32 [n_recordings, k]).  Row r
        is what query_packed_recording_topk_keys_device gives for recording r alone, and what query_packed_topk_keys_device gives
        for query r of the block, bit for bit -- in entry-length steps per pair, all recordings in one pass.  Asynchronous on
        `stream`, nothing visits the host."""
        R, per, k = int(n_recordings), int(per_query), int(k)
        _packed_ok(packed, R, per)
        want_lags = aligned or lags_out is not None
        if keys_out is None or (want_lags and lags_out is None):
            import torch
            dev = packed.device if hasattr(packed, "device") else "cuda"
            with torch.cuda.stream(stream):
                if keys_out is None:
                    keys_out = torch.empty((max(1, R), max(1, k)), dtype=torch.int64, device=dev)
                if want_lags and lags_out is None:
                    lags_out = torch.empty((max(1, R), max(1, k)), dtype=torch.int32, device=dev)
        _out_ok(keys_out, R * k, "keys_out")
        if want_lags:
            _out_ok(lags_out, R * k, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice(
            self._ref, _dev_ptr(packed), R, per, range_, k, index_base, _dev_ptr(keys_out), _dev_ptr(lags_out) if want_lags else None,
            _stream_ptr(stream)), "CorpusQueryPackedRecordingTopKBatchKeysDevice")
        return (keys_out, lags_out) if want_lags else keys_out

    def query_packed_recording_threshold_keys_device(self, packed, per_query: int, threshold: float, capacity: int, range_: int = 0,
                                                     index_base: int = 0, keys_out=None, lags_out=None, count_out=None,
                                                     want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedRecordingThresholdKeysDevice: (keys int64 [capacity], lags int32 [capacity] or None,
        count int64 [1]) on the device for ONE query of per_query packed sub-fingerprints already on the device:
        query_packed_threshold_keys_device's keys (ascending index, 0-padded), true count and aligned lags.  Asynchronous on
        `stream`, nothing visits the host."""
        _packed_ok(packed, 1, per_query)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        keys_out, lags_out, count_out = _occurrences_out(capacity, keys_out, lags_out, count_out, want_lags, dev)
        _check(self._L.LBAudioDetectiveCorpusQueryPackedRecordingThresholdKeysDevice(
            self._ref, _dev_ptr(packed), per_query, range_, threshold, capacity, index_base, _dev_ptr(keys_out), _dev_ptr(count_out),
            _dev_ptr(lags_out) if lags_out is not None else None, _stream_ptr(stream)), "CorpusQueryPackedRecordingThresholdKeysDevice")
        return keys_out, lags_out, count_out

    # ---- batch occurrences and batch recording threshold: every match on every channel at or above a score, in one call
    def _batch_threshold_call(self, which: str, packed, n_recordings, per_query, capacity, keys_out, lags_out, counts_out, want_lags,
                              stream, call):
        R, per, capacity = int(n_recordings), int(per_query), int(capacity)
        _packed_ok(packed, R, per)
        want_lags = want_lags or lags_out is not None
        if keys_out is None or counts_out is None or (want_lags and lags_out is None):
            import torch
            dev = packed.device if hasattr(packed, "device") else "cuda"
            with torch.cuda.stream(stream):              # (the blocks belong to the stream that fills them)
                if keys_out is None:
                    keys_out = torch.empty((max(1, R), max(1, capacity)), dtype=torch.int64, device=dev)
                if want_lags and lags_out is None:
                    lags_out = torch.empty((max(1, R), max(1, capacity)), dtype=torch.int32, device=dev)
                if counts_out is None:
                    counts_out = torch.empty(max(1, R), dtype=torch.int64, device=dev)
        _out_ok(keys_out, R * capacity, "keys_out")
        _out_ok(counts_out, R, "counts_out")
        if want_lags:
            _out_ok(lags_out, R * capacity, "lags_out")
        _check(call(R, per, capacity, _dev_ptr(keys_out), _dev_ptr(lags_out) if want_lags else None, _dev_ptr(counts_out),
                    _stream_ptr(stream)), which)
        return keys_out, (lags_out if want_lags else None), counts_out

    def query_packed_occurrences_batch_keys_device(self, packed, n_recordings: int, per_query: int, threshold: float, capacity: int,
                                                   peaks: bool = False, range_: int = 0, index_base: int = 0, keys_out=None,
                                                   lags_out=None, counts_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice: query_packed_occurrences_keys_device for n_recordings
        recordings of per_query packed sub-fingerprints each, already on the device as [n_recordings, per_query, 32] bytes
        (StreamBank.window_device's block) -> (keys int64 [n_recordings, capacity], lags int32 of the same shape or None, counts
        int64 [n_recordings]) on the device, asynchronously on `stream`.  Row r and counts[r] are what the single call gives for
        recording r alone, bit for bit; a row that overflows touches no other row.  want_lags=False (and no lags_out) passes
        NULL: keys and counts are the same.  Decode rows with decode_occurrence_keys."""
        return self._batch_threshold_call(
            "CorpusQueryPackedOccurrencesBatchKeysDevice", packed, n_recordings, per_query, capacity, keys_out, lags_out, counts_out,
            want_lags, stream,
            lambda R, per, cap, kp, lp, cp, sp: self._L.LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice(
                self._ref, _dev_ptr(packed), R, per, range_, threshold, int(bool(peaks)), cap, index_base, kp, lp, cp, sp))

    def query_packed_recording_threshold_batch_keys_device(self, packed, n_recordings: int, per_query: int, threshold: float,
                                                           capacity: int, range_: int = 0, index_base: int = 0, keys_out=None,
                                                           lags_out=None, counts_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice: query_packed_recording_threshold_keys_device for
        n_recordings recordings of per_query packed sub-fingerprints each -> (keys int64 [n_recordings, capacity], lags int32 of
        the same shape or None, counts int64 [n_recordings]) on the device, asynchronously on `stream`: per recording every entry
        whose best cell reaches `threshold`, in ascending index, with the true count and the aligned lags.  Row r is what the
        single call gives for recording r alone, and what query_packed_threshold_keys_device gives for query r of the block."""
        return self._batch_threshold_call(
            "CorpusQueryPackedRecordingThresholdBatchKeysDevice", packed, n_recordings, per_query, capacity, keys_out, lags_out,
            counts_out, want_lags, stream,
            lambda R, per, cap, kp, lp, cp, sp: self._L.LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice(
                self._ref, _dev_ptr(packed), R, per, range_, threshold, cap, index_base, kp, cp, lp, sp))

    def query_packed_occurrences_tail_batch_keys_device(self, packed, n_recordings: int, per_query: int, new_counts, threshold: float,
                                                        capacity: int, max_new: int = None, range_: int = 0, index_base: int = 0,
                                                        keys_out=None, lags_out=None, counts_out=None, want_lags: bool = True,
                                                        stream=None):
        """LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice: of query_packed_occurrences_batch_keys_device (peaks off)
        only the cells a push has completed -- per recording r those whose entry ends inside its newest d_r = min(new_counts[r],
        max_new, per_query) sub-fingerprints, for the entries not longer than per_query -> (keys int64 [n_recordings, capacity],
        lags int32 of the same shape or None, counts int64 [n_recordings]) on the device, asynchronously on `stream`.  Row r is
        the batch call's row r with only those cells kept, bit for bit; each match of a channel's life is reported once, by the
        call behind the push that completes it.  new_counts: a device uint32 / int32 tensor of n_recordings values (max_new is
        then required: the host's bound, 1 .. 64, which a device value above it is cut to), or a host sequence, uploaded on
        `stream` (max_new defaults to its maximum, at least 1).  Decode with decode_tail_occurrences."""
        R = int(n_recordings)
        if hasattr(new_counts, "data_ptr"):
            import torch
            if max_new is None:
                raise ValueError("max_new is required with new counts on the device")
            if (not new_counts.is_cuda or not new_counts.is_contiguous() or new_counts.dtype not in (torch.int32, torch.uint32) or
                    new_counts.numel() < R):
                raise ValueError("new_counts must be a contiguous device tensor of at least n_recordings uint32 or int32 values")
            d_new = new_counts
        else:
            import torch
            host = np.ascontiguousarray(np.asarray(new_counts).reshape(-1), dtype=np.int64)
            if host.size != R or (host.size and (host.min() < 0 or host.max() > 0xFFFFFFFF)):
                raise ValueError("new_counts must hold one value of 0 .. 2^32 - 1 per recording")
            if max_new is None:
                max_new = max(1, int(host.max()) if host.size else 1)
            dev = packed.device if hasattr(packed, "device") else "cuda"
            with torch.cuda.stream(stream):              # (uploaded on the stream that reads it)
                d_new = torch.from_numpy(host.astype(np.uint32).view(np.int32)).to(dev, non_blocking=False)
        max_new = int(max_new)
        return self._batch_threshold_call(
            "CorpusQueryPackedOccurrencesTailBatchKeysDevice", packed, n_recordings, per_query, capacity, keys_out, lags_out, counts_out,
            want_lags, stream,
            lambda R, per, cap, kp, lp, cp, sp: self._L.LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice(
                self._ref, _dev_ptr(packed), R, per, _dev_ptr(d_new), max_new, range_, threshold, cap, index_base, kp, lp, cp, sp))

    # ---- live best matches: the tail occurrences' cells folded to one value per (recording, entry) -- per-entry scores, the K
    # best, or all at or above a score, of what a push has completed
    @staticmethod
    def _tail_new_counts(packed, n_recordings: int, new_counts, max_new, stream):
        """(device tensor, max_new) of a tail call's new counts, as query_packed_occurrences_tail_batch_keys_device takes them: a
        device uint32 / int32 tensor (max_new required) or a host sequence uploaded on `stream` (max_new defaults to its maximum)"""
        import torch
        R = int(n_recordings)
        if hasattr(new_counts, "data_ptr"):
            if max_new is None:
                raise ValueError("max_new is required with new counts on the device")
            if (not new_counts.is_cuda or not new_counts.is_contiguous() or new_counts.dtype not in (torch.int32, torch.uint32) or
                    new_counts.numel() < R):
                raise ValueError("new_counts must be a contiguous device tensor of at least n_recordings uint32 or int32 values")
            return new_counts, int(max_new)
        host = np.ascontiguousarray(np.asarray(new_counts).reshape(-1), dtype=np.int64)
        if host.size != R or (host.size and (host.min() < 0 or host.max() > 0xFFFFFFFF)):
            raise ValueError("new_counts must hold one value of 0 .. 2^32 - 1 per recording")
        if max_new is None:
            max_new = max(1, int(host.max()) if host.size else 1)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        with torch.cuda.stream(stream):                  # (uploaded on the stream that reads it)
            d_new = torch.from_numpy(host.astype(np.uint32).view(np.int32)).to(dev, non_blocking=False)
        return d_new, int(max_new)

    def query_packed_occurrences_tail_peaks_batch_keys_device(self, packed, n_recordings: int, per_query: int, new_counts,
                                                              threshold: float, capacity: int, max_new: int = None, final: bool = False,
                                                              range_: int = 0, index_base: int = 0, keys_out=None, lags_out=None,
                                                              counts_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice: of query_packed_occurrences_batch_keys_device with
        peaks=True only the cells judged ONE sub-fingerprint late -- per recording r and entry of n_j <= per_query sub-fingerprints
        the offsets max(0, last - d_r) .. last - 1, last = per_query - n_j, d_r = min(new_counts[r], max_new, per_query); with
        final=True the newest cell `last` too (the end of a stream, or before a reset; new count 0 then gives it alone) -> (keys
        int64 [n_recordings, capacity], lags int32 of the same shape or None, counts int64 [n_recordings]) on the device,
        asynchronously on `stream`.  Row r is the batch call's row r with only those cells kept, bit for bit: a plateau reports its
        first cell.  Each peak of a channel's life is reported once when every window holds the whole life so far or at least the
        longest entry + the push's new sub-fingerprints + 1, and one final call closes the stream.  new_counts / max_new as the
        tail occurrences method takes them, max_new 1 .. 62.  Decode with decode_tail_occurrences."""
        d_new, max_new = self._tail_new_counts(packed, int(n_recordings), new_counts, max_new, stream)
        return self._batch_threshold_call(
            "CorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice", packed, n_recordings, per_query, capacity, keys_out, lags_out,
            counts_out, want_lags, stream,
            lambda R, per, cap, kp, lp, cp, sp: self._L.LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice(
                self._ref, _dev_ptr(packed), R, per, _dev_ptr(d_new), max_new, 1 if final else 0, range_, threshold, cap, index_base,
                kp, lp, cp, sp))

    def recording_scores_tail_batch_device(self, packed, n_recordings: int, per_query: int, new_counts, max_new: int = None,
                                           range_: int = 0, scores_out=None, lags_out=None, want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice: the cells of
        query_packed_occurrences_tail_batch_keys_device -- per recording r those whose entry ends inside its newest d_r =
        min(new_counts[r], max_new, per_query) sub-fingerprints -- folded per (recording, entry) -> (scores float32 [n_recordings,
        len(self)], lags int32 of the same shape or None) on the device, asynchronously on `stream`.  scores[r][j] = max(+0, the
        largest q_o of the pair's tail cells), +0 where the pair has none (d_r == 0, an empty entry, an entry longer than
        per_query); lags[r][j] = -(the lowest tail offset that reaches the score), 0 where none does.  Every word is written; an
        empty corpus writes nothing.  new_counts / max_new as the tail occurrences method takes them.  want_lags=False (and no
        lags_out) passes NULL: the scores are the same."""
        R, per = int(n_recordings), int(per_query)
        _packed_ok(packed, R, per)
        d_new, max_new = self._tail_new_counts(packed, R, new_counts, max_new, stream)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        count = len(self)
        n = R * count
        if scores_out is None or (want_lags and lags_out is None):
            import torch
            with torch.cuda.stream(stream):              # (the blocks belong to the stream that fills them)
                if scores_out is None:
                    scores_out = torch.empty(max(1, n), dtype=torch.float32, device=dev)[:n].reshape(R, count)
                if want_lags and lags_out is None:
                    lags_out = torch.empty(max(1, n), dtype=torch.int32, device=dev)[:n].reshape(R, count)
        _out_ok(scores_out, n, "scores_out")
        if lags_out is not None:
            _out_ok(lags_out, n, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice(
            self._ref, _dev_ptr(packed), R, per, _dev_ptr(d_new), max_new, range_, _dev_ptr(scores_out),
            _dev_ptr(lags_out) if lags_out is not None else None, _stream_ptr(stream)), "CorpusRecordingPackedScoresTailBatchDevice")
        return scores_out, lags_out

    def query_packed_recording_topk_tail_batch_keys_device(self, packed, n_recordings: int, per_query: int, new_counts, k: int,
                                                           max_new: int = None, range_: int = 0, index_base: int = 0, keys_out=None,
                                                           lags_out=None, aligned: bool = False, stream=None):
        """LBAudioDetectiveCorpusQueryPackedRecordingTopKTailBatchKeysDevice: the k best entries a push has completed on every
        recording -> the [n_recordings, k] int64 key tensor, and with aligned=True (or a lags_out) (keys, lags int32 [n_recordings,
        k]).  Row r is query_packed_recording_topk_batch_keys_device's selection over row r of
        recording_scores_tail_batch_device: the entries scoring above 0, score descending, the lowest index first among equals,
        zero keys (lag 0) behind them.  A (recording, entry) pair is reported at most once per push, by the push that completes
        its best new cell.  new_counts / max_new as the tail occurrences method takes them.  Asynchronous on `stream`, nothing
        visits the host.  Decode with decode_tail_matches and StreamBank.totals()."""
        R, per, k = int(n_recordings), int(per_query), int(k)
        _packed_ok(packed, R, per)
        d_new, max_new = self._tail_new_counts(packed, R, new_counts, max_new, stream)
        want_lags = aligned or lags_out is not None
        if keys_out is None or (want_lags and lags_out is None):
            import torch
            dev = packed.device if hasattr(packed, "device") else "cuda"
            with torch.cuda.stream(stream):
                if keys_out is None:
                    keys_out = torch.empty((max(1, R), max(1, k)), dtype=torch.int64, device=dev)
                if want_lags and lags_out is None:
                    lags_out = torch.empty((max(1, R), max(1, k)), dtype=torch.int32, device=dev)
        _out_ok(keys_out, R * k, "keys_out")
        if want_lags:
            _out_ok(lags_out, R * k, "lags_out")
        _check(self._L.LBAudioDetectiveCorpusQueryPackedRecordingTopKTailBatchKeysDevice(
            self._ref, _dev_ptr(packed), R, per, _dev_ptr(d_new), max_new, range_, k, index_base, _dev_ptr(keys_out),
            _dev_ptr(lags_out) if want_lags else None, _stream_ptr(stream)), "CorpusQueryPackedRecordingTopKTailBatchKeysDevice")
        return (keys_out, lags_out) if want_lags else keys_out

    def query_packed_recording_threshold_tail_batch_keys_device(self, packed, n_recordings: int, per_query: int, new_counts,
                                                                threshold: float, capacity: int, max_new: int = None, range_: int = 0,
                                                                index_base: int = 0, keys_out=None, lags_out=None, counts_out=None,
                                                                want_lags: bool = True, stream=None):
        """LBAudioDetectiveCorpusQueryPackedRecordingThresholdTailBatchKeysDevice: every entry a push has completed at or above
        `threshold` on every recording -> (keys int64 [n_recordings, capacity], lags int32 of the same shape or None, counts int64
        [n_recordings]) on the device, asynchronously on `stream`.  Row r is
        query_packed_recording_threshold_batch_keys_device's selection over row r of recording_scores_tail_batch_device: ascending
        index, the true count, zeros behind min(count, capacity), lag 0 for a zero key.  It names exactly the distinct entries of
        row r of query_packed_occurrences_tail_batch_keys_device at the same threshold (while that row is not cut), each with the
        key of its largest cell and the lag of the lowest offset that reaches it.  new_counts / max_new as the tail occurrences
        method takes them.  Decode with decode_tail_matches and StreamBank.totals()."""
        d_new, max_new = self._tail_new_counts(packed, int(n_recordings), new_counts, max_new, stream)
        return self._batch_threshold_call(
            "CorpusQueryPackedRecordingThresholdTailBatchKeysDevice", packed, n_recordings, per_query, capacity, keys_out, lags_out,
            counts_out, want_lags, stream,
            lambda R, per, cap, kp, lp, cp, sp: self._L.LBAudioDetectiveCorpusQueryPackedRecordingThresholdTailBatchKeysDevice(
                self._ref, _dev_ptr(packed), R, per, _dev_ptr(d_new), max_new, range_, threshold, cap, index_base, kp, cp, lp, sp))

    # ---- recording timeline: the best entry at every offset of ONE query (a long recording) against a ragged corpus -- the
    # occurrences cells folded per offset over the entries not longer than the query.  One key per sub-fingerprint of the query,
    # whatever the corpus size.  Shards of contiguous index ranges merge by the element-wise maximum of their keys AS UNSIGNED
    # (score bits of a positive float leave the sign bit clear, so torch.maximum on the int64 tensors is that maximum).
    def recording_timeline_keys_device(self, fp: Fingerprint = None, packed=None, per_query: int = 0, threshold: float = 0.0,
                                       range_: int = 0, index_base: int = 0, keys_out=None, lengths_out=None,
                                       want_lengths: bool = True, stream=None):
        """LBAudioDetectiveCorpusRecordingTimelineKeysDevice (fp) / ...RecordingPackedTimelineKeysDevice (packed: per_query packed
        sub-fingerprints already on the device): (keys int64 [n_q], lengths int32 [n_q] or None) on the device, asynchronously on
        `stream`, n_q = the query's sub-fingerprints.  keys[o] is the best cell at or above `threshold` among the entries that
        start at offset o and lie inside the query (score bits << 32 | 0xFFFFFFFF - (index_base + entry), ties to the lower
        entry), 0 where there is none; lengths[o] the winner's sub-fingerprints (the bits of a UInt32; 0 for a zero key).
        want_lengths=False (and no lengths_out) passes NULL: the keys are the same.  Decode with decode_timeline_keys."""
        if (fp is None) == (packed is None):
            raise ValueError("give either fp or packed")
        dev = packed.device if hasattr(packed, "device") else "cuda"
        n = fp.number_of_subfingerprints if fp is not None else int(per_query)
        if keys_out is None or (want_lengths and lengths_out is None):
            import torch
            if keys_out is None:
                keys_out = torch.empty(max(1, n), dtype=torch.int64, device=dev)[:n]
            if want_lengths and lengths_out is None:
                lengths_out = torch.empty(max(1, n), dtype=torch.int32, device=dev)[:n]
        _out_ok(keys_out, n, "keys_out")
        if lengths_out is not None:
            _out_ok(lengths_out, n, "lengths_out")
        lp = _dev_ptr(lengths_out) if lengths_out is not None else None
        if fp is not None:
            _check(self._L.LBAudioDetectiveCorpusRecordingTimelineKeysDevice(self._ref, fp._ref, range_, threshold, index_base,
                                                                            _dev_ptr(keys_out), lp, _stream_ptr(stream)),
                   "CorpusRecordingTimelineKeysDevice")
        else:
            _packed_ok(packed, 1, per_query)
            _check(self._L.LBAudioDetectiveCorpusRecordingPackedTimelineKeysDevice(self._ref, _dev_ptr(packed), per_query, range_,
                                                                                  threshold, index_base, _dev_ptr(keys_out), lp,
                                                                                  _stream_ptr(stream)),
                   "CorpusRecordingPackedTimelineKeysDevice")
        return keys_out, lengths_out

    def recording_timeline_batch_keys_device(self, packed, n_recordings: int, per_query: int, threshold: float, range_: int = 0,
                                             index_base: int = 0, keys_out=None, lengths_out=None, want_lengths: bool = True,
                                             stream=None):
        """LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice: the timeline of n_recordings recordings of per_query packed
        sub-fingerprints each, already on the device as [n_recordings, per_query, 32] bytes (StreamBank.window_device's block) ->
        (keys int64 [n_recordings, per_query], lengths int32 [n_recordings, per_query] or None) on the device, asynchronously on
        `stream`.  Row r is what recording_timeline_keys_device gives for recording r alone, bit for bit.  want_lengths=False (and
        no lengths_out) passes NULL: the keys are the same.  Decode with decode_timeline_batch_keys."""
        R, per = int(n_recordings), int(per_query)
        _packed_ok(packed, R, per)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        n = R * per
        if keys_out is None or (want_lengths and lengths_out is None):
            import torch
            if keys_out is None:
                keys_out = torch.empty(max(1, n), dtype=torch.int64, device=dev)[:n].reshape(R, per)
            if want_lengths and lengths_out is None:
                lengths_out = torch.empty(max(1, n), dtype=torch.int32, device=dev)[:n].reshape(R, per)
        _out_ok(keys_out, n, "keys_out")
        if lengths_out is not None:
            _out_ok(lengths_out, n, "lengths_out")
        _check(self._L.LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice(
            self._ref, _dev_ptr(packed), R, per, range_, threshold, index_base, _dev_ptr(keys_out),
            _dev_ptr(lengths_out) if lengths_out is not None else None, _stream_ptr(stream)), "CorpusRecordingPackedTimelineBatchKeysDevice")
        return keys_out, lengths_out

    def recording_timeline_tail_batch_keys_device(self, packed, n_recordings: int, per_query: int, new_counts, threshold: float,
                                                  max_new: int = None, prev_keys=None, keys_out=None, lengths_out=None,
                                                  want_lengths: bool = True, range_: int = 0, index_base: int = 0, stream=None):
        """LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice: the timeline of n_recordings windows AFTER a push from
        the timeline before it -> (keys int64 [n_recordings, per_query], lengths int32 of the same shape or None) on the device,
        asynchronously on `stream`.  keys[r][o] is the unsigned maximum of prev_keys[r][o + min(new_counts[r], per_query)] (0
        beyond the row, or without prev_keys) and the best cell at or above `threshold` among the cells the push completed at
        offset o: the entries that end inside the newest min(new_counts[r], max_new, per_query) sub-fingerprints, keyed as
        recording_timeline_batch_keys_device keys them; lengths[r][o] is the length of the entry the key names (0 for a zero key
        or an index outside the corpus).  Seeded with recording_timeline_batch_keys_device and called after every push whose
        counts are <= max_new, the output equals that call on the new windows, bit for bit.  A count above max_new shifts by the
        true count but adds only the newest max_new cells: seed again instead (LiveTimeline does).  prev_keys must not overlap
        keys_out.  new_counts / max_new as the tail occurrences method takes them.  want_lengths=False (and no lengths_out)
        passes NULL: the keys are the same.  Shards of contiguous index ranges merge by torch.maximum of their keys.  Decode
        with decode_timeline_batch_keys."""
        R, per = int(n_recordings), int(per_query)
        _packed_ok(packed, R, per)
        d_new, max_new = self._tail_new_counts(packed, R, new_counts, max_new, stream)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        n = R * per
        if prev_keys is not None:
            _out_ok(prev_keys, n, "prev_keys")
        if keys_out is None or (want_lengths and lengths_out is None):
            import torch
            with torch.cuda.stream(stream):              # (the blocks belong to the stream that fills them)
                if keys_out is None:
                    keys_out = torch.empty(max(1, n), dtype=torch.int64, device=dev)[:n].reshape(R, per)
                if want_lengths and lengths_out is None:
                    lengths_out = torch.empty(max(1, n), dtype=torch.int32, device=dev)[:n].reshape(R, per)
        _out_ok(keys_out, n, "keys_out")
        if lengths_out is not None:
            _out_ok(lengths_out, n, "lengths_out")
        _check(self._L.LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice(
            self._ref, _dev_ptr(packed), R, per, _dev_ptr(d_new), max_new, range_, threshold, index_base,
            _dev_ptr(prev_keys) if prev_keys is not None else None, _dev_ptr(keys_out),
            _dev_ptr(lengths_out) if lengths_out is not None else None, _stream_ptr(stream)),
            "CorpusRecordingPackedTimelineTailBatchKeysDevice")
        return keys_out, lengths_out

    def recording_segments_batch_keys_device(self, packed, n_recordings: int, per_query: int, threshold: float, capacity: int,
                                             range_: int = 0, index_base: int = 0, stream=None):
        """What played when in n_recordings recordings at once: recording_timeline_batch_keys_device, then
        timeline_segments_device on its output, on ONE stream with nothing in between (per_query <= 8192).  Returns (starts int32,
        keys int64, lengths int32, all [n_recordings, capacity], counts int32 [n_recordings]) on the device: row r holds the
        non-overlapping spans of recording r in start order, zeros behind them; counts are never cut.  Decode with
        decode_segments(..., index_base).  The timeline's keys and lengths in between are allocated under `stream`, like the
        outputs: they are dropped on return while `stream` may still use them, and only a block that belongs to `stream` is
        handed out again behind that work."""
        import torch
        R, per = int(n_recordings), int(per_query)
        dev = packed.device if hasattr(packed, "device") else "cuda"
        with torch.cuda.stream(stream):                  # (the blocks belong to the stream that fills them)
            keys = torch.empty(max(1, R * per), dtype=torch.int64, device=dev)[:R * per].reshape(R, per)
            lengths = torch.empty(max(1, R * per), dtype=torch.int32, device=dev)[:R * per].reshape(R, per)
        self.recording_timeline_batch_keys_device(packed, R, per, threshold, range_=range_, index_base=index_base, keys_out=keys,
                                                  lengths_out=lengths, stream=stream)
        return timeline_segments_device(keys, lengths, capacity, stream=stream)

    def recording_timeline(self, fp: Fingerprint, threshold: float, range_: int = 0):
        """LBAudioDetectiveCorpusQueryRecordingTimeline: (indices int64[n_q], scores float32[n_q], lengths uint32[n_q]) per offset
        of the query: the best entry at or above `threshold` that starts there and lies inside the query, its score and its
        sub-fingerprints; -1 / 0 / 0 where there is none."""
        n = fp.number_of_subfingerprints
        idx = np.full(max(1, n), -1, dtype=np.int64)
        sc = np.zeros(max(1, n), dtype=np.float32)
        ln = np.zeros(max(1, n), dtype=np.uint32)
        cnt = N.UInt64(0)
        _check(self._L.LBAudioDetectiveCorpusQueryRecordingTimeline(self._ref, fp._ref, range_, threshold,
                                                                   idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                                   sc.ctypes.data_as(C.POINTER(N.Float32)),
                                                                   ln.ctypes.data_as(C.POINTER(N.UInt32)), C.byref(cnt)),
               "CorpusQueryRecordingTimeline")
        return idx[:n].copy(), sc[:n].copy(), ln[:n].copy()

    def recording_segments(self, fp: Fingerprint, threshold: float, range_: int = 0):
        """What played when: (start, index, score, length) arrays of non-overlapping spans [start, start + length) of the query,
        sorted by start -- timeline_segments of recording_timeline's result.  GREEDY over the per-offset WINNERS, not over all
        cells: an entry that is second best at its offset is never reported, even where the winner there is later suppressed by
        an overlapping better span."""
        return timeline_segments(*self.recording_timeline(fp, threshold, range_))

    def entry_lengths_from_keys_device(self, keys, index_base: int = 0, out=None, stream=None):
        """LBAudioDetectiveCorpusEntryLengthsFromKeysDevice: 64-bit keys on the device, exactly as every key call writes them -> an
        int32 device tensor in the keys' shape (the bits of a UInt32): the sub-fingerprints of the entry each key names, 0 for a
        zero key or an index outside [index_base, index_base + len(self)).  What occurrence_segments_device takes as lengths; a
        shard serves the keys of its own range.  Asynchronous on `stream`."""
        import torch
        assert keys.is_cuda and keys.is_contiguous() and keys.element_size() == 8
        n = keys.numel()
        if out is None:
            with torch.cuda.stream(stream):              # (the block belongs to the stream that fills it)
                out = torch.empty(max(1, n), dtype=torch.int32, device=keys.device)[:n].reshape(keys.shape)
        assert out.element_size() == 4
        _out_ok(out, n, "out")
        _check(self._L.LBAudioDetectiveCorpusEntryLengthsFromKeysDevice(self._ref, _dev_ptr(keys), n, index_base, _dev_ptr(out),
                                                                       _stream_ptr(stream)), "CorpusEntryLengthsFromKeysDevice")
        return out

    def recording_occurrence_segments_batch_keys_device(self, packed, n_recordings: int, per_query: int, threshold: float, capacity: int,
                                                        out_capacity: int, peaks: bool = True, range_: int = 0, index_base: int = 0,
                                                        stream=None):
        """What played when in n_recordings recordings at once, over ALL matching cells: query_packed_occurrences_batch_keys_device
        (rows of `capacity` slots, <= 8192; with peaks one cell per airing), entry_lengths_from_keys_device on its keys, then
        occurrence_segments_device, on ONE stream with nothing read back (per_query <= 8192).  Returns (starts int32, keys int64,
        lags int32, lengths int32, all [n_recordings, out_capacity], counts int32 [n_recordings], occurrence_counts int64
        [n_recordings]) on the device: row r holds the non-overlapping spans of recording r in start order, zeros behind them;
        counts are never cut.  occurrence_counts are the occurrences call's own: where occurrence_counts[r] > capacity the row
        was CUT in (entry, offset) order before the greedy ran, and its spans are those of the cells that were kept -- raise the
        capacity or the threshold.  Decode with decode_occurrence_segments(..., index_base).  The blocks in between are allocated
        under `stream`, like the outputs."""
        R, per = int(n_recordings), int(per_query)
        keys, lags, occ_counts = self.query_packed_occurrences_batch_keys_device(packed, R, per, threshold, capacity, peaks=peaks,
                                                                                 range_=range_, index_base=index_base, stream=stream)
        lengths = self.entry_lengths_from_keys_device(keys, index_base=index_base, stream=stream)
        return occurrence_segments_device(keys, lags, lengths, occ_counts, per, out_capacity, stream=stream) + (occ_counts,)

    def recording_occurrence_segments(self, fp: Fingerprint, threshold: float, range_: int = 0, peaks: bool = True):
        """What played when, over ALL matching cells: (start, index, score, lag, length) arrays of non-overlapping spans of the
        query sorted by start -- occurrence_segments of the query's occurrences (with peaks, the default, one cell per airing),
        computed on the device and decoded.  Where recording_segments sees the best entry per offset only, this reports the second
        best at an offset when the winner there loses to a better overlapping span.  The query has at most 8192 sub-fingerprints;
        more than 8192 matching cells raise ValueError: raise the threshold or keep peaks on."""
        n = fp.number_of_subfingerprints
        cap = N.OCCURRENCE_SEGMENTS_MAX_CANDIDATES
        if not 1 <= n <= N.SEGMENTS_MAX_SUBFINGERPRINTS:
            raise ValueError(f"the query must have 1 .. {N.SEGMENTS_MAX_SUBFINGERPRINTS} sub-fingerprints")
        keys, lags, count = self.query_occurrences_keys_device(fp, threshold, cap, peaks=peaks, range_=range_)
        lengths = self.entry_lengths_from_keys_device(keys)
        rows = occurrence_segments_device(keys, lags, lengths, count, n, n)
        if int(count.cpu().reshape(-1)[0]) > cap:
            raise ValueError(f"more than {cap} matching cells: raise the threshold or use peaks")
        return decode_occurrence_segments(*rows)

    def set_join_scratch_limit(self, n_bytes: int):
        """bytes of device memory the join's scratch may take, and thereby the rows per chunk; 0 restores the default"""
        _check(self._L.LBAudioDetectiveCorpusSetJoinScratchLimit(self._ref, n_bytes), "CorpusSetJoinScratchLimit")

    # ---- removal: the named entries go, the others keep their order and close up (old index i -> i - removed below i); the
    # corpus is afterwards what a fresh one would be after appending the kept entries.  Synchronous calls.
    def remove(self, indices, return_map: bool = False):
        """LBAudioDetectiveCorpusRemoveIndices: remove the entries at `indices` (host integers, duplicates allowed; an index >=
        len(self) is refused and nothing changes).  Returns the number of distinct entries removed, or with return_map=True
        (removed, uint32 array with one word per OLD entry: its new index, 0xFFFFFFFF for a removed entry)."""
        idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.uint64)
        new = np.full(max(1, len(self)), 0xFFFFFFFF, dtype=np.uint32) if return_map else None
        n_old, removed = len(self), N.UInt64(0)
        _check(self._L.LBAudioDetectiveCorpusRemoveIndices(self._ref, idx.ctypes.data_as(C.POINTER(N.UInt64)) if idx.size else None,
                                                          idx.size, new.ctypes.data_as(C.POINTER(N.UInt32)) if return_map else None,
                                                          C.byref(removed)), "CorpusRemoveIndices")
        return (int(removed.value), new[:n_old].copy()) if return_map else int(removed.value)

    def remove_keys_device(self, keys, index_base: int = 0, new_indices_out=None, stream=None) -> int:
        """LBAudioDetectiveCorpusRemoveKeysDevice: remove the entries named by 64-bit keys on the device, exactly as the top-K,
        threshold and join calls write them (global index = index_base + local; zero keys and keys of other entries are skipped,
        duplicates allowed).  new_indices_out: an int32 / uint32 device tensor of len(self) words that receives the map.  The
        kernels run on `stream` (the stream that produced the keys); the call returns when they are done."""
        assert keys.is_cuda and keys.is_contiguous() and keys.element_size() == 8
        n = keys.numel()
        if new_indices_out is not None:
            assert new_indices_out.element_size() == 4
            _out_ok(new_indices_out, len(self), "new_indices_out")
        removed = N.UInt64(0)
        _check(self._L.LBAudioDetectiveCorpusRemoveKeysDevice(self._ref, _dev_ptr(keys) if n else None, n, index_base,
                                                             _dev_ptr(new_indices_out) if new_indices_out is not None else None,
                                                             C.byref(removed), _stream_ptr(stream)), "CorpusRemoveKeysDevice")
        return int(removed.value)

    def set_remove_scratch_limit(self, n_bytes: int):
        """bytes of device memory a removal's bounce buffer may take, and thereby the entries (records) per chunk; 0 restores
        the default"""
        _check(self._L.LBAudioDetectiveCorpusSetRemoveScratchLimit(self._ref, n_bytes), "CorpusSetRemoveScratchLimit")

    # ---- gather: entries handed back in the packed layout (Boolean b at bit b & 31 of word b >> 5, 32 bytes per sub-fingerprint),
    # row i = element i of the list, with the rows' offsets: offsets[i + 1] - offsets[i] sub-fingerprints, offsets[-1] the total.
    def gather_keys_device(self, keys, index_base: int = 0, packed_out=None, offsets_out=None, capacity=None, stream=None):
        """LBAudioDetectiveCorpusGatherKeysDevice: the entries named by 64-bit keys on the device, exactly as the top-K, threshold
        and join calls write them (global index = index_base + local; a zero key or a key of another entry is an empty row,
        duplicates yield copies) -> (packed uint8 [capacity, 32], offsets int64 [len(keys) + 1]) on the device, asynchronously on
        `stream`.  Positions at or above the capacity are not written; offsets[-1] is the true total either way.  With neither
        capacity nor packed_out given the call sizes itself first (the sizing call and one read-back of the total)."""
        import torch
        assert keys.is_cuda and keys.is_contiguous() and keys.element_size() == 8
        n = keys.numel()
        sp = _stream_ptr(stream)
        if offsets_out is None:
            offsets_out = torch.empty(n + 1, dtype=torch.int64, device=keys.device)
        _out_ok(offsets_out, n + 1, "offsets_out")
        fn = self._L.LBAudioDetectiveCorpusGatherKeysDevice
        if capacity is None:
            if packed_out is not None:
                capacity = packed_out.numel() * packed_out.element_size() // N.PACKED_BYTES
            else:
                _check(fn(self._ref, _dev_ptr(keys) if n else None, n, index_base, None, 0, _dev_ptr(offsets_out), sp),
                       "CorpusGatherKeysDevice")
                if stream is not None:
                    stream.synchronize()
                else:
                    torch.cuda.current_stream().synchronize()
                capacity = int(offsets_out[n].item())
        if packed_out is None:
            packed_out = torch.empty((capacity, N.PACKED_BYTES), dtype=torch.uint8, device=keys.device)
        if not packed_out.is_cuda or not packed_out.is_contiguous() or packed_out.numel() * packed_out.element_size() < capacity * N.PACKED_BYTES:
            raise ValueError("packed_out must be a contiguous device tensor of at least capacity * 32 bytes")
        _check(fn(self._ref, _dev_ptr(keys) if n else None, n, index_base, _dev_ptr(packed_out) if capacity else None, capacity,
                  _dev_ptr(offsets_out), sp), "CorpusGatherKeysDevice")
        return packed_out, offsets_out

    def gather(self, indices):
        """LBAudioDetectiveCorpusGatherIndices: the entries at `indices` (host integers, duplicates allowed; an index >= len(self)
        is refused) -> numpy (packed uint8 [total, 32], offsets uint64 [len(indices) + 1])."""
        idx = np.ascontiguousarray(np.asarray(indices).reshape(-1), dtype=np.uint64)
        n = idx.size
        ip = idx.ctypes.data_as(C.POINTER(N.UInt64)) if n else None
        offsets = np.zeros(n + 1, dtype=np.uint64)
        op = offsets.ctypes.data_as(C.POINTER(N.UInt64))
        _check(self._L.LBAudioDetectiveCorpusGatherIndices(self._ref, ip, n, None, 0, op), "CorpusGatherIndices")
        total = int(offsets[n])
        packed = np.zeros((total, N.PACKED_BYTES), dtype=np.uint8)
        if total:
            _check(self._L.LBAudioDetectiveCorpusGatherIndices(self._ref, ip, n, packed.ctypes.data, total, op), "CorpusGatherIndices")
        return packed, offsets

    # ---- entry ids: the caller's own 64-bit id of every entry (0: none), on the device with the entry: it moves with it through
    # removals, is saved with it, comes back for any key list and names entries in the key format the taking calls read.
    @property
    def has_entry_ids(self) -> bool:
        """LBAudioDetectiveCorpusHasEntryIds: ids were set (or loaded) at some time; a corpus starts without."""
        return bool(self._L.LBAudioDetectiveCorpusHasEntryIds(self._ref))

    def set_entry_ids(self, ids, first: int = 0, stream=None):
        """LBAudioDetectiveCorpusSetEntryIdsDevice / ...SetEntryIds: entries [first, first + len(ids)) get these ids.  ids: a
        contiguous device tensor of 8-byte elements (asynchronous on `stream`) or host integers (copied before the call returns;
        `stream` is ignored).  A range beyond len(self) is refused and nothing changes; an empty list does not turn ids on."""
        if hasattr(ids, "is_cuda") and ids.is_cuda:
            assert ids.is_contiguous() and ids.element_size() == 8
            n = ids.numel()
            _check(self._L.LBAudioDetectiveCorpusSetEntryIdsDevice(self._ref, first, n, _dev_ptr(ids) if n else None, _stream_ptr(stream)),
                   "CorpusSetEntryIdsDevice")
        else:
            host = np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.uint64)
            _check(self._L.LBAudioDetectiveCorpusSetEntryIds(self._ref, first, host.size,
                                                            host.ctypes.data_as(C.POINTER(N.UInt64)) if host.size else None),
                   "CorpusSetEntryIds")
        return self

    def entry_ids(self, first: int = 0, n=None) -> np.ndarray:
        """LBAudioDetectiveCorpusGetEntryIds: the ids of entries [first, first + n) as numpy uint64 (n None: up to len(self));
        zeros for a corpus without ids.  The range may reach up to the capacity: the words from len(self) on are zero."""
        if n is None:
            n = max(0, len(self) - first)
        out = np.zeros(n, dtype=np.uint64)
        _check(self._L.LBAudioDetectiveCorpusGetEntryIds(self._ref, first, n, out.ctypes.data_as(C.POINTER(N.UInt64)) if n else None),
               "CorpusGetEntryIds")
        return out

    def ids_from_keys_device(self, keys, index_base: int = 0, out=None, stream=None):
        """LBAudioDetectiveCorpusIdsFromKeysDevice: 64-bit keys on the device, exactly as the top-K, threshold, join, occurrences,
        recording, timeline and group calls write them -> an int64 device tensor of keys.numel() ids (the id's 64 bits): 0 for
        a zero key, a key of another entry, or a corpus without ids.  Asynchronous on `stream`."""
        import torch
        assert keys.is_cuda and keys.is_contiguous() and keys.element_size() == 8
        n = keys.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=keys.device)
        assert out.element_size() == 8
        _out_ok(out, n, "out")
        _check(self._L.LBAudioDetectiveCorpusIdsFromKeysDevice(self._ref, _dev_ptr(keys) if n else None, n, index_base,
                                                              _dev_ptr(out) if n else None, _stream_ptr(stream)), "CorpusIdsFromKeysDevice")
        return out

    def keys_from_ids_device(self, ids, index_base: int = 0, out=None, stream=None):
        """LBAudioDetectiveCorpusKeysFromIdsDevice: 64-bit ids on the device -> an int64 device tensor of ids.numel() keys in list
        order: score word 1.0f, low word 0xFFFFFFFF - (index_base + index) of the LOWEST index with that id; the zero key for
        id 0, an id no entry has, or a corpus without ids.  remove_keys_device, gather_keys_device and align_keys_device take
        the result as it is.  Asynchronous on `stream`; the first call after ids were set, a removal or a load builds the index."""
        import torch
        assert ids.is_cuda and ids.is_contiguous() and ids.element_size() == 8
        n = ids.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=ids.device)
        assert out.element_size() == 8
        _out_ok(out, n, "out")
        _check(self._L.LBAudioDetectiveCorpusKeysFromIdsDevice(self._ref, _dev_ptr(ids) if n else None, n, index_base,
                                                              _dev_ptr(out) if n else None, _stream_ptr(stream)), "CorpusKeysFromIdsDevice")
        return out

    def _ids_tensor(self, ids):
        import torch
        if hasattr(ids, "is_cuda") and ids.is_cuda:
            return ids
        return torch.from_numpy(np.ascontiguousarray(np.asarray(ids).reshape(-1), dtype=np.uint64).view(np.int64)).cuda()

    def remove_ids(self, ids, stream=None) -> int:
        """take-down by id: keys_from_ids_device, then remove_keys_device.  Of entries that share an id the one at the lowest
        index goes; ids no entry has are skipped.  Returns the number of entries removed."""
        return self.remove_keys_device(self.keys_from_ids_device(self._ids_tensor(ids), stream=stream), stream=stream)

    def gather_ids(self, ids, stream=None):
        """hand-back by id: keys_from_ids_device, then gather_keys_device -> (packed, offsets) on the device, row i = ids[i] (an
        empty row for an id no entry has)."""
        return self.gather_keys_device(self.keys_from_ids_device(self._ids_tensor(ids), stream=stream), stream=stream)

    def fingerprint(self, index: int) -> Fingerprint:
        """LBAudioDetectiveCorpusCopyFingerprint: entry `index` as a new host Fingerprint (IndexError for index >= len(self))."""
        if not 0 <= index < len(self):
            raise IndexError(f"entry {index} of a corpus of {len(self)}")
        ref = self._L.LBAudioDetectiveCorpusCopyFingerprint(self._ref, index)
        if not ref:
            raise LBAudioDetectiveError(1, "CorpusCopyFingerprint")
        return Fingerprint(_ref=ref)

    # ---- duplicate groups: the connected components of the self-join's match graph (a match in either direction joins two
    # entries), and the removal of everything except each group's first entry.  Composites in Python over the device calls, as
    # identify_clips_device is; uniform corpora of the join's shape and ragged corpora (the ragged join), the joins refuse the rest.
    def duplicate_groups(self, threshold: float, key_capacity: int = 1 << 22, rows_per_call=None, range_: int = 0, stream=None):
        """(labels int32 [len(self)], group_count int64 [1]) on the device: labels[i] is the lowest index of the entries that
        entry i is connected to through pairs scoring >= threshold in either direction (see group_labels_from_keys_device).  A
        self-join with skip_same_index in chunks of rows, each chunk's keys grouped into the one labels tensor.  Each chunk's
        total is read back; a chunk whose total exceeds key_capacity is redone with half the rows (a multiple of 64 while there
        are 64 or more), and a single row that does not fit raises ValueError: the result never rests on a cut list and
        depends on neither key_capacity nor rows_per_call."""
        import torch
        n = len(self)
        if key_capacity < 1:
            raise ValueError("key_capacity must be at least 1")
        labels = torch.empty(max(1, n), dtype=torch.int32, device="cuda")[:n]
        groups = torch.zeros(1, dtype=torch.int64, device="cuda")
        if n == 0:
            return labels, groups
        rows = n if rows_per_call is None else max(1, min(int(rows_per_call), n))
        keys = torch.empty(key_capacity, dtype=torch.int64, device="cuda")
        offsets = torch.empty(rows + 1, dtype=torch.int64, device="cuda")
        ragged = self.subfingerprints_per_entry == 0       # (Corpus.ragged: entries of any length)
        first, reset = 0, True
        while first < n:
            count = min(rows, n - first)
            while True:
                if ragged:
                    self.join_ragged_threshold_keys_device(threshold, key_capacity, first=first, count=count, skip_same_index=True,
                                                           range_=range_, keys_out=keys, offsets_out=offsets, want_lags=False,
                                                           stream=stream)
                else:
                    self.join_threshold_keys_device(threshold, key_capacity, first=first, count=count, skip_same_index=True,
                                                    range_=range_, keys_out=keys, offsets_out=offsets, stream=stream)
                if stream is not None:
                    stream.synchronize()
                total = int(offsets[count].item())         # (the one read-back of a chunk: its true total)
                if total <= key_capacity:
                    break
                if count == 1:
                    raise ValueError(f"row {first} alone has {total} matches: key_capacity {key_capacity} is too small")
                count = count // 2 // 64 * 64 if count >= 128 else max(1, count // 2)
                rows = count                               # (it stays: the rows behind are likely as dense)
            group_labels_from_keys_device(keys, n, offsets=offsets, n_rows=count, first_row=first, labels=labels, reset=reset,
                                          group_count=groups, n_slots=min(total, key_capacity), stream=stream)
            reset = False
            first += count
        return labels, groups

    def deduplicate(self, threshold: float, key_capacity: int = 1 << 22, rows_per_call=None, range_: int = 0, stream=None):
        """duplicate_groups, then the keys of every entry that is not its group's first, then remove_keys_device: one entry per
        group stays, the first.  Returns (removed, labels_before): the number of entries removed and the labels over the OLD
        indices."""
        labels, _ = self.duplicate_groups(threshold, key_capacity=key_capacity, rows_per_call=rows_per_call, range_=range_, stream=stream)
        if len(self) == 0:
            return 0, labels
        keys, count = group_extra_keys_from_labels_device(labels, stream=stream)
        removed = self.remove_keys_device(keys[:count], stream=stream) if count else 0
        return removed, labels

    # ---- where a match lies (LBAudioDetectiveCorpusQueryAligned and kin): lag > 0, the query's sub-fingerprint 0 lines up
    # with the entry's sub-fingerprint lag (the entry is the longer one); lag < 0, the entry's sub-fingerprint 0 lines up with
    # the query's sub-fingerprint -lag; 0 for equal lengths and for empty slots.  Positions in seconds: lag x 128 x analysis
    # stride / processing sample rate (PCM entry points).
    def query_aligned(self, fp: Fingerprint, range_: int = 0):
        """query()'s (index, score), bit for bit, plus the winner's lag."""
        idx, score, lag = N.SInt64(-1), N.Float32(0.0), N.SInt32(0)
        _check(self._L.LBAudioDetectiveCorpusQueryAligned(self._ref, fp._ref, range_, C.byref(idx), C.byref(score), C.byref(lag)),
               "CorpusQueryAligned")
        return int(idx.value), float(score.value), int(lag.value)

    def query_topk_aligned(self, fp: Fingerprint, k: int, range_: int = 0):
        """query_topk()'s (indices, scores) plus every match's lag (int32)."""
        return self.query_batch_topk_aligned([fp], k, range_)[0]

    def query_batch_topk_aligned(self, fps, k: int, range_: int = 0):
        """query_batch_topk() with lags -> list of (indices, scores, lags); indices and scores are query_batch_topk's."""
        n = len(fps)
        refs = (N.Ref * max(1, n))(*[f._ref for f in fps])
        idx = np.full((max(1, n), max(1, k)), -1, dtype=np.int64)
        sc = np.zeros((max(1, n), max(1, k)), dtype=np.float32)
        lag = np.zeros((max(1, n), max(1, k)), dtype=np.int32)
        cnt = np.zeros(max(1, n), dtype=np.uint32)
        _check(self._L.LBAudioDetectiveCorpusQueryBatchTopKAligned(self._ref, refs, n, range_, k,
                                                                   idx.ctypes.data_as(C.POINTER(N.SInt64)),
                                                                   sc.ctypes.data_as(C.POINTER(N.Float32)),
                                                                   lag.ctypes.data_as(C.POINTER(N.SInt32)),
                                                                   cnt.ctypes.data_as(C.POINTER(N.UInt32))), "CorpusQueryBatchTopKAligned")
        return [(idx[i, :cnt[i]].copy(), sc[i, :cnt[i]].copy(), lag[i, :cnt[i]].copy()) for i in range(n)]

    def align_keys_device(self, fps, keys, k: int, index_base: int = 0, stream=None, want_scores: bool = False, range_: int = 0):
        """LBAudioDetectiveCorpusAlignKeysDevice: the lags of len(fps) x k keys (torch int64 on the device, rows as
        query_batch_topk_keys_device writes them) -> torch int32 [len(fps), k] on the device, asynchronously on `stream`; with
        want_scores also the recomputed float32 scores.  Zero keys and indices outside this corpus get lag 0 and score 0."""
        import torch
        n = len(fps)
        if keys.numel() < n * k or not keys.is_contiguous() or keys.dtype != torch.int64:
            raise ValueError("keys must be a contiguous int64 tensor of at least len(fps) * k keys")
        refs = (N.Ref * max(1, n))(*[f._ref for f in fps])
        lags = torch.empty((max(1, n), k), dtype=torch.int32, device=keys.device)
        scores = torch.empty((max(1, n), k), dtype=torch.float32, device=keys.device) if want_scores else None
        _check(self._L.LBAudioDetectiveCorpusAlignKeysDevice(self._ref, refs, n, range_, k, keys.data_ptr(), index_base,
                                                             lags.data_ptr(), scores.data_ptr() if want_scores else None,
                                                             _stream_ptr(stream)), "CorpusAlignKeysDevice")
        return (lags, scores) if want_scores else lags

    def match_profile(self, fp: Fingerprint, entry: int, range_: int = 0):
        """Every offset's score of fp against entry `entry` (LBAudioDetectiveCorpusMatchProfile) -> (float32 array, first_lag):
        slot o lies at lag first_lag + o when the entry is longer than the query, first_lag - o otherwise; the maximum is the
        entry's score."""
        count, first = N.UInt64(0), N.SInt32(0)
        st = self._L.LBAudioDetectiveCorpusMatchProfile(self._ref, fp._ref, range_, entry, None, 0, C.byref(count), C.byref(first))
        if count.value == 0:                  # (a capacity of 0 is too small for any pair: only a refused call leaves it 0)
            _check(st, "CorpusMatchProfile")
        out = np.zeros(count.value, dtype=np.float32)
        _check(self._L.LBAudioDetectiveCorpusMatchProfile(self._ref, fp._ref, range_, entry, out.ctypes.data_as(C.POINTER(N.Float32)),
                                                          out.size, C.byref(count), C.byref(first)), "CorpusMatchProfile")
        return out, int(first.value)

    @staticmethod
    def decode_key(key: int):
        idx, score = N.SInt64(-1), N.Float32(0.0)
        N.lib().LBAudioDetectiveCorpusDecodeKey(key & 0xFFFFFFFFFFFFFFFF, C.byref(idx), C.byref(score))
        return int(idx.value), float(score.value)


def _dev_ptr(x):
    """device address of a torch tensor, or the raw address itself"""
    return C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else C.c_void_p(int(x))


def _packed_ok(packed, n_queries: int, per_query: int):
    if hasattr(packed, "data_ptr"):
        if not packed.is_cuda or not packed.is_contiguous() or packed.numel() * packed.element_size() < n_queries * per_query * N.PACKED_BYTES:
            raise ValueError("packed must be a contiguous device tensor of at least n_queries * per_query * 32 bytes")


def _out_ok(out, n: int, what: str):
    if hasattr(out, "data_ptr") and (not out.is_cuda or not out.is_contiguous() or out.numel() < n):
        raise ValueError(f"{what} must be a contiguous device tensor of at least {n} elements")


def _threshold_out(n: int, capacity: int, keys_out, counts_out, lags_out, want_lags: bool, device):
    """the outputs of a threshold call on the device: made where they are missing, checked where they are given"""
    if keys_out is None or counts_out is None or (want_lags and lags_out is None):
        import torch
        if keys_out is None:
            keys_out = torch.empty((max(1, n), max(1, capacity)), dtype=torch.int64, device=device)
        if counts_out is None:
            counts_out = torch.empty(max(1, n), dtype=torch.int64, device=device)
        if want_lags and lags_out is None:
            lags_out = torch.empty((max(1, n), max(1, capacity)), dtype=torch.int32, device=device)
    _out_ok(keys_out, n * capacity, "keys_out")
    _out_ok(counts_out, n, "counts_out")
    if want_lags:
        _out_ok(lags_out, n * capacity, "lags_out")
    return keys_out, counts_out, lags_out


def _occurrences_out(capacity: int, keys_out, lags_out, count_out, want_lags: bool, device):
    """the outputs of an occurrences call on the device: made where they are missing, checked where they are given"""
    if keys_out is None or count_out is None or (want_lags and lags_out is None):
        import torch
        if keys_out is None:
            keys_out = torch.empty(max(1, capacity), dtype=torch.int64, device=device)
        if count_out is None:
            count_out = torch.empty(1, dtype=torch.int64, device=device)
        if want_lags and lags_out is None:
            lags_out = torch.empty(max(1, capacity), dtype=torch.int32, device=device)
    _out_ok(keys_out, capacity, "keys_out")
    _out_ok(count_out, 1, "count_out")
    if lags_out is not None:
        _out_ok(lags_out, capacity, "lags_out")
    return keys_out, lags_out, count_out


def identify_clips_device(det: "Detective", corpus: "Corpus", clips, k: int = 1, aligned: bool = False, range_: int = 0, stream=None):
    """Clips on the device -> their k best corpus matches on the device: Detective.fingerprint_clips_device, then
    Corpus.query_packed_topk_keys_device on its output, on ONE stream with nothing in between (no handle, no copy to the host,
    no synchronisation).  Returns the [n, k] int64 key tensor (decode rows with decode_topk_keys), and with aligned=True
    (keys, lags int32 [n, k])."""
    packed = det.fingerprint_clips_device(clips, stream=stream)
    n, per = packed.shape[0], packed.shape[1]
    return corpus.query_packed_topk_keys_device(packed, n, per, k, aligned=aligned, range_=range_, stream=stream)


def debug_query_blocks(kind: int, n_queries: int, per_query: int, subfp_len: int, range_: int = 0, packed=None, bools=None) -> np.ndarray:
    """LBAudioDetectiveDebugQueryBlocks (tests): the query blocks as uint32 [n_queries, words] -- built on the device from
    `packed` (device tensor or address) or on the host from `bools` ([n_queries, per_query, subfp_len]).  kind 0: specialised
    uniform scan, 1: ragged scan, 2 / 3: alignment words of a ragged / uniform corpus."""
    count = N.UInt64(0)
    b = _u8(bools) if bools is not None else None
    if b is not None and b.size != n_queries * per_query * subfp_len:
        raise ValueError("bools must hold n_queries x per_query x subfp_len Booleans")
    src = (_dev_ptr(packed) if packed is not None else None, b.ctypes.data if b is not None else None)
    L = N.lib()
    L.LBAudioDetectiveDebugQueryBlocks(kind, src[0], src[1], n_queries, per_query, subfp_len, range_, None, 0, C.byref(count))
    out = np.zeros(max(1, count.value), np.uint32)
    _check(L.LBAudioDetectiveDebugQueryBlocks(kind, src[0], src[1], n_queries, per_query, subfp_len, range_, out.ctypes.data, out.size,
                                              C.byref(count)), "DebugQueryBlocks")
    return out[:count.value].reshape(n_queries, -1)


SLIDING_CHOICE_WORDS = 21


def debug_sliding_choice(hist, n_pos: int, ne_max: int, variant: int, subfp_len: int, n_query: int, n_left: int, range_: int = 0,
                         scores: bool = False, host_blocks: bool = True, cus: int = 256) -> list:
    """LBAudioDetectiveDebugSlidingChoice (tests): the kernel one launch of a ragged scan takes, as the 21 words the header
    describes.  hist: (entry length, count) pairs.  Needs no device."""
    lengths = (N.UInt32 * max(1, len(hist)))(*[int(h[0]) for h in hist])
    counts = (N.UInt64 * max(1, len(hist)))(*[int(h[1]) for h in hist])
    out = (N.UInt32 * SLIDING_CHOICE_WORDS)()
    _check(N.lib().LBAudioDetectiveDebugSlidingChoice(lengths, counts, len(hist), n_pos, ne_max, variant, subfp_len, n_query, n_left,
                                                      range_, int(bool(scores)), int(bool(host_blocks)), cus, out, SLIDING_CHOICE_WORDS),
           "DebugSlidingChoice")
    return list(out)


def debug_live_bytes():
    """LBAudioDetectiveDebugLiveBytes (tests): (device, pinned) bytes that detectives and corpora hold right now."""
    dev, pinned = N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugLiveBytes(C.byref(dev), C.byref(pinned)), "DebugLiveBytes")
    return dev.value, pinned.value


def debug_set_grid_ceiling(workgroups: int) -> None:
    """LBAudioDetectiveDebugSetGridCeiling (tests only): at most `workgroups` workgroups for every launch that walks its work
    items with a grid stride and LDS state carried between them; 0 restores the built-in ceilings.  Results never depend on it."""
    _check(N.lib().LBAudioDetectiveDebugSetGridCeiling(int(workgroups)), "DebugSetGridCeiling")


def debug_grid_ceiling():
    """LBAudioDetectiveDebugGridCeiling (tests): (the ceiling, launches of this process so far whose grid was below their work)."""
    n, strided = N.UInt32(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugGridCeiling(C.byref(n), C.byref(strided)), "DebugGridCeiling")
    return n.value, strided.value


def debug_timeline_batch_plan(n_recordings: int, per_query: int, shortest_entry: int, longest_entry: int, entries: int,
                              scratch_limit: int = 0) -> dict:
    """LBAudioDetectiveDebugTimelineBatchPlan: the host plan of one batch timeline call -- the one the call itself takes -- as a
    dict: form (0: S, the shared window; 1: W, a window per wave), tiles per recording, recordings_per_pass, entries_per_chunk,
    scratch_bytes of a pass, lds_bytes of a workgroup.  scratch_limit 0: the default.  Raises for a shape or limit the call
    refuses.  Needs no GPU."""
    form, rpp = N.UInt32(0), N.UInt32(0)
    tiles, chunk, scratch, lds = N.UInt64(0), N.UInt64(0), N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugTimelineBatchPlan(int(n_recordings), int(per_query), int(shortest_entry), int(longest_entry),
                                                          int(entries), int(scratch_limit), C.byref(form), C.byref(tiles), C.byref(rpp),
                                                          C.byref(chunk), C.byref(scratch), C.byref(lds)), "DebugTimelineBatchPlan")
    return {"form": form.value, "tiles": tiles.value, "recordings_per_pass": rpp.value, "entries_per_chunk": chunk.value,
            "scratch_bytes": scratch.value, "lds_bytes": lds.value}


def debug_set_timeline_batch_form(force_shared: bool) -> None:
    """LBAudioDetectiveDebugSetTimelineBatchForm (measurements and tests): True makes every later batch timeline plan take form S
    where form W would be chosen, False restores the choice.  Results never depend on it."""
    _check(N.lib().LBAudioDetectiveDebugSetTimelineBatchForm(1 if force_shared else 0), "DebugSetTimelineBatchForm")


def debug_recording_batch_plan(n_recordings: int, per_query: int, shortest_entry: int, longest_entry: int, entries: int,
                               scratch_limit: int = 0, key_form: bool = False) -> dict:
    """LBAudioDetectiveDebugRecordingBatchPlan: the host plan of one batch recording scores call (key_form=True: of one batch
    recording top-K call) -- the one the call itself takes -- as a dict: form (0: S, the shared window; 1: W, a window per wave),
    tiles per recording, recordings_per_pass, entries_per_chunk, scratch_bytes of a pass, lds_bytes of a workgroup.
    scratch_limit 0: the default.  Raises for a shape or limit the call refuses.  Needs no GPU."""
    form, rpp = N.UInt32(0), N.UInt32(0)
    tiles, chunk, scratch, lds = N.UInt64(0), N.UInt64(0), N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugRecordingBatchPlan(int(n_recordings), int(per_query), int(shortest_entry), int(longest_entry),
                                                           int(entries), int(scratch_limit), 1 if key_form else 0, C.byref(form),
                                                           C.byref(tiles), C.byref(rpp), C.byref(chunk), C.byref(scratch), C.byref(lds)),
           "DebugRecordingBatchPlan")
    return {"form": form.value, "tiles": tiles.value, "recordings_per_pass": rpp.value, "entries_per_chunk": chunk.value,
            "scratch_bytes": scratch.value, "lds_bytes": lds.value}


def debug_set_recording_batch_form(force_shared: bool) -> None:
    """LBAudioDetectiveDebugSetRecordingBatchForm (measurements and tests): True makes every later batch recording plan take form S
    where form W would be chosen, False restores the choice; the batch timeline's switch is another.  Results never depend on it."""
    _check(N.lib().LBAudioDetectiveDebugSetRecordingBatchForm(1 if force_shared else 0), "DebugSetRecordingBatchForm")


def debug_occurrences_batch_plan(n_recordings: int, per_query: int, shortest_entry: int, longest_entry: int, entries: int,
                                 scratch_limit: int = 0) -> dict:
    """LBAudioDetectiveDebugOccurrencesBatchPlan: the host plan of one batch occurrences call -- the one the call itself takes --
    as a dict: form (0: S, the shared window; 1: W, a window per wave), tiles per recording, recordings_per_pass,
    entries_per_chunk, scratch_bytes of a pass, lds_bytes of a workgroup.  scratch_limit 0: the default.  Raises for a shape or
    limit the call refuses.  Needs no GPU."""
    form, rpp = N.UInt32(0), N.UInt32(0)
    tiles, chunk, scratch, lds = N.UInt64(0), N.UInt64(0), N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugOccurrencesBatchPlan(int(n_recordings), int(per_query), int(shortest_entry), int(longest_entry),
                                                             int(entries), int(scratch_limit), C.byref(form), C.byref(tiles),
                                                             C.byref(rpp), C.byref(chunk), C.byref(scratch), C.byref(lds)),
           "DebugOccurrencesBatchPlan")
    return {"form": form.value, "tiles": tiles.value, "recordings_per_pass": rpp.value, "entries_per_chunk": chunk.value,
            "scratch_bytes": scratch.value, "lds_bytes": lds.value}


def debug_set_occurrences_batch_form(force_shared: bool) -> None:
    """LBAudioDetectiveDebugSetOccurrencesBatchForm (measurements and tests): True makes every later plan of the batch occurrences
    and the batch recording threshold take form S where form W would be chosen, False restores the choice; the other batch
    calls' switches are others.  Results never depend on it."""
    _check(N.lib().LBAudioDetectiveDebugSetOccurrencesBatchForm(1 if force_shared else 0), "DebugSetOccurrencesBatchForm")


def debug_occurrences_tail_plan(n_recordings: int, per_query: int, shortest_entry: int, longest_entry: int, entries: int, max_new: int,
                                scratch_limit: int = 0) -> dict:
    """LBAudioDetectiveDebugOccurrencesTailPlan: the host plan of one tail occurrences call -- the one the call itself takes -- as
    a dict: lanes per recording, recordings_per_workgroup, window_records of a recording in LDS, lds_bytes of a workgroup,
    recordings_per_pass, entries_per_chunk, scratch_bytes of a pass.  scratch_limit 0: the default.  Raises for a shape or limit
    the call refuses.  Needs no GPU."""
    lanes, rpw, win, rpp = N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt32(0)
    lds, chunk, scratch = N.UInt64(0), N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugOccurrencesTailPlan(int(n_recordings), int(per_query), int(shortest_entry), int(longest_entry),
                                                            int(entries), int(max_new), int(scratch_limit), C.byref(lanes), C.byref(rpw),
                                                            C.byref(win), C.byref(lds), C.byref(rpp), C.byref(chunk), C.byref(scratch)),
           "DebugOccurrencesTailPlan")
    return {"lanes": lanes.value, "recordings_per_workgroup": rpw.value, "window_records": win.value, "lds_bytes": lds.value,
            "recordings_per_pass": rpp.value, "entries_per_chunk": chunk.value, "scratch_bytes": scratch.value}


def debug_occurrences_tail_peaks_plan(n_recordings: int, per_query: int, shortest_entry: int, longest_entry: int, entries: int,
                                      max_new: int, scratch_limit: int = 0) -> dict:
    """LBAudioDetectiveDebugOccurrencesTailPeaksPlan: the host plan of one tail peaks call -- the one the call itself takes -- with
    debug_occurrences_tail_plan's fields: it is that plan at max_new + 2 (a recording's lanes hold the two neighbour cells),
    max_new 1 .. 62.  Needs no GPU."""
    lanes, rpw, win, rpp = N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt32(0)
    lds, chunk, scratch = N.UInt64(0), N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugOccurrencesTailPeaksPlan(int(n_recordings), int(per_query), int(shortest_entry),
                                                                 int(longest_entry), int(entries), int(max_new), int(scratch_limit),
                                                                 C.byref(lanes), C.byref(rpw), C.byref(win), C.byref(lds), C.byref(rpp),
                                                                 C.byref(chunk), C.byref(scratch)),
           "DebugOccurrencesTailPeaksPlan")
    return {"lanes": lanes.value, "recordings_per_workgroup": rpw.value, "window_records": win.value, "lds_bytes": lds.value,
            "recordings_per_pass": rpp.value, "entries_per_chunk": chunk.value, "scratch_bytes": scratch.value}


def debug_recording_tail_plan(n_recordings: int, per_query: int, longest_entry: int, entries: int, max_new: int, scratch_limit: int = 0,
                              key_form: bool = False) -> dict:
    """LBAudioDetectiveDebugRecordingTailPlan: the host plan of one recording tail call (scores form, or with key_form the top-K
    and threshold forms) -- the one the calls themselves take -- as a dict: lanes per recording, recordings_per_workgroup,
    window_records of a recording in LDS, lds_bytes of a workgroup (those four are debug_occurrences_tail_plan's),
    recordings_per_pass, scratch_bytes of a pass (the key forms' score and lag rows).  scratch_limit 0: the default.  Raises for a
    shape the call refuses.  Needs no GPU."""
    lanes, rpw, win, rpp = N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt32(0)
    lds, scratch = N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugRecordingTailPlan(int(n_recordings), int(per_query), int(longest_entry), int(entries), int(max_new),
                                                          int(scratch_limit), 1 if key_form else 0, C.byref(lanes), C.byref(rpw),
                                                          C.byref(win), C.byref(lds), C.byref(rpp), C.byref(scratch)),
           "DebugRecordingTailPlan")
    return {"lanes": lanes.value, "recordings_per_workgroup": rpw.value, "window_records": win.value, "lds_bytes": lds.value,
            "recordings_per_pass": rpp.value, "scratch_bytes": scratch.value}


def debug_timeline_tail_plan(n_recordings: int, per_query: int, shortest_entry: int, longest_entry: int, entries: int, max_new: int,
                             scratch_limit: int = 0) -> dict:
    """LBAudioDetectiveDebugTimelineTailPlan: the host plan of one timeline tail call -- the one the call itself takes -- as a dict:
    lanes per recording and window_records of a recording in LDS (debug_occurrences_tail_plan's), strip_width (the 64-bit
    accumulators of a recording: min(longest_entry, per_query) - shortest_entry + lanes; 0 where no entry takes part),
    recordings_per_workgroup (fewer than the tail plan's where the strips do not fit beside the windows), lds_bytes of a workgroup,
    recordings_per_pass, scratch_bytes of a pass (its strips).  scratch_limit 0: the default.  Raises for a shape the call refuses
    or a limit below one recording's strip.  Needs no GPU."""
    lanes, rpw, win, width, rpp = N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt32(0), N.UInt32(0)
    lds, scratch = N.UInt64(0), N.UInt64(0)
    _check(N.lib().LBAudioDetectiveDebugTimelineTailPlan(int(n_recordings), int(per_query), int(shortest_entry), int(longest_entry),
                                                         int(entries), int(max_new), int(scratch_limit), C.byref(lanes), C.byref(rpw),
                                                         C.byref(win), C.byref(width), C.byref(lds), C.byref(rpp), C.byref(scratch)),
           "DebugTimelineTailPlan")
    return {"lanes": lanes.value, "recordings_per_workgroup": rpw.value, "window_records": win.value, "strip_width": width.value,
            "lds_bytes": lds.value, "recordings_per_pass": rpp.value, "scratch_bytes": scratch.value}


class LiveTimeline:
    """The timeline of the n most recent sub-fingerprints of the listed channels of a StreamBank, kept current from each push:
    what StreamBank.timeline(corpus, channels, n, threshold, ...) returns after every push, bit for bit, for the work of the
    push's new cells alone.  The state is two pairs of device buffers that take turns; nothing is kept in the bank or the corpus,
    and nothing is read back.  The CALLER calls reseed() after entries were removed from the corpus (the keys name indices) or a
    listed channel was reset; entries appended to the corpus count from the push behind them on, for the cells that push
    completes -- reseed() to have them judged against the whole window."""

    def __init__(self, bank: "StreamBank", corpus: "Corpus", channels, n: int, threshold: float, max_new: int = 8, range_: int = 0,
                 index_base: int = 0):
        self.bank, self.corpus = bank, corpus
        self.channels = _u32_list(channels)[0].copy()
        self.n, self.threshold, self.max_new = int(n), float(threshold), int(max_new)
        self.range_, self.index_base = int(range_), int(index_base)
        if not 1 <= self.max_new <= 64:
            raise ValueError("max_new must be 1 .. 64")
        self._state = None                               # (keys, lengths) of the latest update
        self._spare = None                               # the pair the next update writes

    def reseed(self) -> None:
        """The next update computes the whole timeline again (StreamBank.timeline)."""
        self._state = None

    def update(self, new_counts, stream=None):
        """After a push: new_counts is what push / push_device returned (one value per channel of the BANK, on the host).
        Returns (keys int64 [len(channels), n], lengths int32 of the same shape) on the device, asynchronously on `stream`: the
        current timeline.  The first call, the call after reseed() and any call where a listed channel's count exceeds max_new
        go through StreamBank.timeline; every other call is window_device and
        Corpus.recording_timeline_tail_batch_keys_device from the previous state, on ONE stream with nothing in between.  The
        tensors returned are the state: they are read by the next update and written again by the one after it."""
        mine = np.asarray(new_counts).reshape(-1)[self.channels].astype(np.int64)
        out = self._spare
        if self._state is None or (mine.size and int(mine.max()) > self.max_new):
            packed = self.bank.window_device(self.channels, self.n, stream=stream)
            fresh = self.corpus.recording_timeline_batch_keys_device(
                packed, packed.shape[0], self.n, self.threshold, range_=self.range_, index_base=self.index_base,
                keys_out=out[0] if out else None, lengths_out=out[1] if out else None, stream=stream)
        else:
            packed = self.bank.window_device(self.channels, self.n, stream=stream)
            fresh = self.corpus.recording_timeline_tail_batch_keys_device(
                packed, packed.shape[0], self.n, mine, self.threshold, max_new=self.max_new, prev_keys=self._state[0],
                keys_out=out[0] if out else None, lengths_out=out[1] if out else None, range_=self.range_,
                index_base=self.index_base, stream=stream)
        self._spare, self._state = self._state, fresh
        return fresh

    def segments(self, capacity: int, stream=None):
        """timeline_segments_device on the current state: what StreamBank.segments returns for the same windows."""
        if self._state is None:
            raise RuntimeError("LiveTimeline.segments before the first update")
        return timeline_segments_device(self._state[0], self._state[1], capacity, stream=stream)


class Comm:
    """An RCCL communicator made through the library's helpers (ncclCommInitRank with the current device).
    `unique_id()` on rank 0, the 128 bytes travel to the other ranks by whatever means the host has, then every
    rank constructs Comm(n_ranks, unique_id, rank)."""

    UNIQUE_ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.UNIQUE_ID_BYTES)
        _check(N.lib().LBAudioDetectiveCommGetUniqueId(buf), "CommGetUniqueId")
        return buf.raw

    def __init__(self, n_ranks: int, unique_id: bytes, rank: int):
        assert len(unique_id) == Comm.UNIQUE_ID_BYTES
        self._L = N.lib()
        self.n_ranks, self.rank = n_ranks, rank
        ref = C.c_void_p()
        _check(self._L.LBAudioDetectiveCommInitRank(C.byref(ref), n_ranks, unique_id, rank), "CommInitRank")
        self._ref = ref

    def info(self):
        """(ranks that joined the communicator, this rank's number in it) -- ncclCommCount / ncclCommUserRank."""
        n, r = N.SInt32(0), N.SInt32(0)
        _check(self._L.LBAudioDetectiveCommGetInfo(self._ref, C.byref(n), C.byref(r)), "CommGetInfo")
        return int(n.value), int(r.value)

    def dispose(self):
        if getattr(self, "_ref", None):
            self._L.LBAudioDetectiveCommDestroy(self._ref)
            self._ref = None

    def __del__(self):
        try:
            self.dispose()
        except Exception:
            pass


def read_audio_url(path: str, sample_rate: float = 0.0, resampler: int = 0):
    """Decode a CAF/WAV file to mono float32 (numpy), optionally resampled; returns (samples, rate)."""
    buf, n, rate = C.POINTER(N.Float32)(), N.UInt64(0), N.Float64(0.0)
    _check(N.lib().LBAudioDetectiveReadAudioURLWithResampler(path.encode(), float(sample_rate), int(resampler),
                                                             C.byref(buf), C.byref(n), C.byref(rate)), "ReadAudioURL")
    try:
        out = np.ctypeslib.as_array(buf, shape=(n.value,)).copy() if n.value else np.zeros(0, np.float32)
    finally:
        N.lib().LBAudioDetectiveFreeSamples(buf)
    return out, float(rate.value)


def probe_shader_clock(stream=None, microseconds: int = 2000) -> float:
    """Shader clock in MHz over `microseconds`, measured by a one-wave kernel on `stream` (use a side stream to
    read the clock under another kernel's load); synchronises that stream."""
    mhz = N.Float64(0.0)
    _check(N.lib().LBAudioDetectiveProbeShaderClock(_stream_ptr(stream), microseconds, C.byref(mhz)), "ProbeShaderClock")
    return float(mhz.value)


def synth_clips_device(seed: int, first: int, n_clips: int, sample_rate_hz: int, n_samples: int,
                       stereo_sum: bool = False, out=None, stream=None):
    import torch
    if out is None:
        out = torch.empty((n_clips, n_samples), dtype=torch.float32, device="cuda")
    _check(N.lib().LBAudioDetectiveSynthClipsDevice(seed & 0xFFFFFFFF, first, n_clips, sample_rate_hz, n_samples,
                                                    int(stereo_sum), out.data_ptr(), _stream_ptr(stream)),
           "SynthClipsDevice")
    return out


def synth_ragged_corpus_device(seed: int, first: int, counts, subfp_len: int, stream=None):
    """Synthetic ragged corpus on the device: entry first + e has counts[e] sub-fingerprints (lbo_synth_entry's);
    returns packed uint8 [sum(counts), 32]."""
    import torch
    cnt = np.ascontiguousarray(counts, dtype=np.uint32)
    off = np.zeros(cnt.size + 1, np.uint32)
    np.cumsum(cnt, out=off[1:])
    total = int(off[-1])
    d_off = torch.from_numpy(off.view(np.int32)).cuda()
    out = torch.empty((total, N.PACKED_BYTES), dtype=torch.uint8, device="cuda")
    _check(N.lib().LBAudioDetectiveSynthRaggedCorpusDevice(seed & 0xFFFFFFFF, first, cnt.size, d_off.data_ptr(), total,
                                                           subfp_len, out.data_ptr(), _stream_ptr(stream)),
           "SynthRaggedCorpusDevice")
    torch.cuda.current_stream().synchronize() if stream is None else stream.synchronize()   # d_off is a temporary
    return out


def topk_keys_from_scores_device(scores, k: int, index_base: int = 0, stream=None):
    """LBAudioDetectiveTopKKeysFromScoresDevice: the k largest (score, ~index) keys of every row of `scores` (torch float32 on
    the device, [n] or [rows, n]) -> torch int64 [rows, k] (or [k]), rows descending, 0-padded; scores <= 0 or NaN are never
    selected."""
    import torch
    s = scores.contiguous()
    rows, n = (1, s.numel()) if s.dim() == 1 else (s.shape[0], s.shape[1])
    out = torch.empty((rows, k), dtype=torch.int64, device=s.device)
    _check(N.lib().LBAudioDetectiveTopKKeysFromScoresDevice(s.data_ptr(), n, rows, k, index_base, out.data_ptr(),
                                                            _stream_ptr(stream)), "TopKKeysFromScoresDevice")
    return out[0] if s.dim() == 1 else out


def decode_topk_keys(keys):
    """(indices int64[n], scores float32[n]) of one row of top-K keys (any int64 sequence; zero keys are padding)."""
    k = np.asarray(keys.cpu().numpy() if hasattr(keys, "cpu") else keys, dtype=np.int64).astype(np.uint64)
    k = k[k != 0]
    return (0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64), (k >> np.uint64(32)).astype(np.uint32).view(np.float32)


def threshold_keys_from_scores_device(scores, threshold: float, capacity: int, index_base: int = 0, keys_out=None, counts_out=None,
                                      stream=None):
    """LBAudioDetectiveThresholdKeysFromScoresDevice: per row of `scores` (torch float32 on the device, [n] or [rows, n]) the keys
    of the positions whose score is >= threshold, in ascending position, cut at `capacity`, 0-padded -> (keys int64 [rows,
    capacity], counts int64 [rows]) (or ([capacity], scalar tensor) for a 1-d input); the counts are never cut."""
    s = scores if scores.is_contiguous() else scores.contiguous()
    rows, n = (1, s.numel()) if s.dim() == 1 else (s.shape[0], s.shape[1])
    keys_out, counts_out, _ = _threshold_out(rows, capacity, keys_out, counts_out, None, False, s.device)
    _check(N.lib().LBAudioDetectiveThresholdKeysFromScoresDevice(s.data_ptr(), n, rows, threshold, capacity, index_base,
                                                                 _dev_ptr(keys_out), _dev_ptr(counts_out), _stream_ptr(stream)),
           "ThresholdKeysFromScoresDevice")
    return (keys_out[0], counts_out[0]) if s.dim() == 1 else (keys_out, counts_out)


def decode_threshold_keys(row, count=None):
    """(indices int64[m], scores float32[m]) of one row of threshold keys (any int64 sequence), m = min(count, len(row)) -- or,
    without a count, the keys in front of the zero padding.  The order is the row's: ascending index."""
    k = np.asarray(row.cpu().numpy() if hasattr(row, "cpu") else row, dtype=np.int64).astype(np.uint64).reshape(-1)
    k = k[k != 0] if count is None else k[:min(int(count), len(k))]
    return (0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64), (k >> np.uint64(32)).astype(np.uint32).view(np.float32)


def decode_occurrence_keys(keys, lags=None, count=None):
    """(indices int64[m], scores float32[m], lags int32[m] or None) of an occurrences call's keys (any int64 sequence), m =
    min(count, len(keys)) -- or, without a count, the keys in front of the zero padding.  The order is the call's."""
    k = np.asarray(keys.cpu().numpy() if hasattr(keys, "cpu") else keys, dtype=np.int64).astype(np.uint64).reshape(-1)
    m = int(np.count_nonzero(k)) if count is None else min(int(count), len(k))
    k = k[:m]
    lg = None
    if lags is not None:
        lg = np.asarray(lags.cpu().numpy() if hasattr(lags, "cpu") else lags, dtype=np.int32).reshape(-1)[:m].copy()
    return ((0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64), (k >> np.uint64(32)).astype(np.uint32).view(np.float32), lg)


def decode_tail_occurrences(keys, lags, counts, totals, n: int, index_base: int = 0):
    """The rows of a tail occurrences call (Corpus.query_packed_occurrences_tail_batch_keys_device, StreamBank.new_occurrences) as a
    list with one (indices int64[m], scores float32[m], starts int64[m]) per recording, m = min(counts[r], capacity): the entry's
    index (global minus index_base), the cell's score and the ABSOLUTE sub-fingerprint at which the match starts in the
    recording's life, totals[r] - n - lag, with totals[r] the recording's sub-fingerprints so far (StreamBank.totals() of the
    listed channels) and n the call's window.  keys / lags: [recordings, capacity], any int sequence or device tensor."""
    k = np.asarray(keys.cpu().numpy() if hasattr(keys, "cpu") else keys, dtype=np.int64)
    lg = np.asarray(lags.cpu().numpy() if hasattr(lags, "cpu") else lags, dtype=np.int32)
    cn = np.asarray(counts.cpu().numpy() if hasattr(counts, "cpu") else counts).reshape(-1).astype(np.int64)
    tt = np.asarray(totals).reshape(-1).astype(np.int64)
    k = k.reshape(cn.size, -1)
    lg = lg.reshape(cn.size, -1)
    if tt.size != cn.size:
        raise ValueError("totals must have one value per recording")
    rows = []
    for r in range(cn.size):
        idx, sc, lag = decode_occurrence_keys(k[r], lg[r], cn[r])
        rows.append((idx - int(index_base), sc, tt[r] - int(n) - lag.astype(np.int64)))
    return rows


def decode_tail_matches(keys, lags, totals, n: int, counts=None, index_base: int = 0):
    """The rows of a recording tail key call (Corpus.query_packed_recording_topk_tail_batch_keys_device,
    ...threshold_tail_batch_keys_device, StreamBank.new_best, StreamBank.new_matches_above) as a list with one (indices int64[m],
    scores float32[m], starts int64[m]) per recording: the entry's index (global minus index_base), the score of its best new
    cell and the ABSOLUTE sub-fingerprint at which that cell starts in the recording's life, totals[r] - n - lag.  m =
    min(counts[r], slots) with the threshold call's counts; with counts=None the non-zero keys of a row count (the top-K call's
    rows, or a threshold row).  keys / lags: [recordings, slots], any int sequence or device tensor."""
    tt = np.asarray(totals).reshape(-1).astype(np.int64)
    k = np.asarray(keys.cpu().numpy() if hasattr(keys, "cpu") else keys, dtype=np.int64).reshape(tt.size, -1)
    lg = np.asarray(lags.cpu().numpy() if hasattr(lags, "cpu") else lags, dtype=np.int32).reshape(tt.size, -1)
    cn = None
    if counts is not None:
        cn = np.asarray(counts.cpu().numpy() if hasattr(counts, "cpu") else counts).reshape(-1).astype(np.int64)
        if cn.size != tt.size:
            raise ValueError("counts must have one value per recording")
    rows = []
    for r in range(tt.size):
        idx, sc, lag = decode_occurrence_keys(k[r], lg[r], None if cn is None else cn[r])
        rows.append((idx - int(index_base), sc, tt[r] - int(n) - lag.astype(np.int64)))
    return rows


def decode_timeline_keys(keys, lengths=None, index_base: int = 0):
    """(indices int64[n], scores float32[n], lengths uint32[n] or None) of a timeline call's keys (any int64 sequence), one per
    offset of the query: -1 / 0 / 0 for a zero key, the entry's index (global minus index_base) otherwise."""
    k = np.asarray(keys.cpu().numpy() if hasattr(keys, "cpu") else keys, dtype=np.int64).astype(np.uint64).reshape(-1)
    idx = np.where(k != 0, (0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64) - int(index_base), -1).astype(np.int64)
    sc = (k >> np.uint64(32)).astype(np.uint32).view(np.float32)
    ln = None
    if lengths is not None:
        ln = np.asarray(lengths.cpu().numpy() if hasattr(lengths, "cpu") else lengths).reshape(-1).astype(np.int64).astype(np.uint32)
    return idx, sc, ln


def decode_timeline_batch_keys(keys, lengths=None, index_base: int = 0):
    """decode_timeline_keys for a batch call's 2-D keys (and lengths): the same three arrays in the keys' own shape
    [recordings, offsets], row r what decode_timeline_keys gives for row r."""
    shape = tuple(keys.shape)
    idx, sc, ln = decode_timeline_keys(keys, lengths, index_base)
    return idx.reshape(shape), sc.reshape(shape), (ln.reshape(shape) if ln is not None else None)

def timeline_segments(indices, scores, lengths):
    """Non-overlapping spans from a timeline's per-offset winners (indices -1 where there is none): the winners are visited in
    descending key order (higher score, then lower index), ties to the lower offset, and a winner at offset o is accepted when
    [o, o + length) meets no accepted span.  Returns (start int64[m], index int64[m], score float32[m], length uint32[m]) sorted
    by start.  Greedy over the WINNERS, not over all cells."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    sc = np.asarray(scores, dtype=np.float32).reshape(-1)
    ln = np.asarray(lengths, dtype=np.uint32).reshape(-1)
    at = np.flatnonzero(idx >= 0)
    # (descending score, ascending index, ascending offset; lexsort's last key is the primary one)
    order = at[np.lexsort((at, idx[at], -sc[at].astype(np.float64)))]
    taken = np.zeros(len(idx) + 1, dtype=bool)
    kept = []
    for o in order:
        end = min(int(o) + int(ln[o]), len(idx))
        if ln[o] == 0 or taken[o:end].any():
            continue
        taken[o:end] = True
        kept.append(int(o))
    kept = np.asarray(sorted(kept), dtype=np.int64)
    return kept, idx[kept], sc[kept], ln[kept]


def timeline_segments_device(keys, lengths, capacity: int, starts_out=None, keys_out=None, lengths_out=None, counts_out=None,
                             want_lengths: bool = True, stream=None):
    """LBAudioDetectiveTimelineSegmentsFromKeysDevice: timeline_segments on the device, for the keys and lengths of one recording
    ([n], as recording_timeline_keys_device returns them) or of a batch ([recordings, n], as recording_timeline_batch_keys_device
    and StreamBank.timeline return them; n <= 8192) -> (starts int32 [recordings, capacity], keys int64 [recordings, capacity],
    lengths int32 of that shape or None, counts int32 [recordings]) on the device, asynchronously on `stream`; for 1-D input the
    rows themselves ([capacity], ..., a scalar tensor).  A row holds its recording's non-overlapping spans in start order, the
    keys unchanged -- ids_from_keys_device, gather_keys_device, align_keys_device, remove_keys_device and decode_threshold_keys
    read the key block as it is -- zeros behind them; counts are the true numbers of spans, never cut at `capacity`.
    want_lengths=False (and no lengths_out) passes NULL: the other outputs are the same.  Decode with decode_segments."""
    if keys.dim() not in (1, 2) or tuple(lengths.shape) != tuple(keys.shape):
        raise ValueError("keys and lengths must be 1-D or 2-D tensors of one shape")
    import torch
    if not (keys.is_cuda and keys.is_contiguous() and lengths.is_cuda and lengths.is_contiguous()
            and keys.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
            and lengths.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))):
        raise ValueError("keys (int64 or uint64) and lengths (int32 or uint32) must be contiguous device tensors")
    R, per = (1, keys.shape[0]) if keys.dim() == 1 else (keys.shape[0], keys.shape[1])
    cap = int(capacity)
    if starts_out is None or keys_out is None or counts_out is None or (want_lengths and lengths_out is None):
        with torch.cuda.stream(stream):                 # (the blocks belong to the stream that fills them)
            shape = (max(1, R), max(1, cap))
            if starts_out is None:
                starts_out = torch.empty(shape, dtype=torch.int32, device=keys.device)
            if keys_out is None:
                keys_out = torch.empty(shape, dtype=torch.int64, device=keys.device)
            if want_lengths and lengths_out is None:
                lengths_out = torch.empty(shape, dtype=torch.int32, device=keys.device)
            if counts_out is None:
                counts_out = torch.empty(max(1, R), dtype=torch.int32, device=keys.device)
    _out_ok(starts_out, R * cap, "starts_out")
    _out_ok(keys_out, R * cap, "keys_out")
    _out_ok(counts_out, R, "counts_out")
    if lengths_out is not None:
        _out_ok(lengths_out, R * cap, "lengths_out")
    _check(N.lib().LBAudioDetectiveTimelineSegmentsFromKeysDevice(
        _dev_ptr(keys), _dev_ptr(lengths), R, per, cap, _dev_ptr(starts_out), _dev_ptr(keys_out),
        _dev_ptr(lengths_out) if lengths_out is not None else None, _dev_ptr(counts_out), _stream_ptr(stream)),
        "TimelineSegmentsFromKeysDevice")
    if keys.dim() == 1:                                  # (outputs given as [capacity] or [1, capacity]: the row either way)
        def row(x):
            return x.reshape(-1)[:cap] if hasattr(x, "reshape") else x
        return (row(starts_out), row(keys_out), (row(lengths_out) if lengths_out is not None else None),
                counts_out.reshape(-1)[0] if hasattr(counts_out, "reshape") else counts_out)
    return starts_out, keys_out, lengths_out, counts_out


def decode_segments(starts, keys, lengths, counts, index_base: int = 0):
    """The rows of timeline_segments_device on the host: per recording the (start int64[m], index int64[m], score float32[m],
    length uint32[m]) arrays timeline_segments returns, m = min(count, capacity); a list with one tuple per recording, or the one
    tuple for 1-D rows.  Without lengths the last array is None."""
    def host(x, dtype):
        return np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x).astype(dtype)

    k = host(keys, np.int64).astype(np.uint64)
    one = k.ndim == 1
    k = k.reshape(1, -1) if one else k
    st = host(starts, np.int64).reshape(k.shape)
    ln = host(lengths, np.int64).astype(np.uint32).reshape(k.shape) if lengths is not None else None
    cnt = host(counts, np.int64).reshape(-1)
    out = []
    for r in range(k.shape[0]):
        m = min(int(cnt[r]), k.shape[1])
        idx = (0xFFFFFFFF - (k[r, :m] & np.uint64(0xFFFFFFFF))).astype(np.int64) - int(index_base)
        sc = (k[r, :m] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out.append((st[r, :m].copy(), idx, sc, ln[r, :m].copy() if ln is not None else None))
    return out[0] if one else out


def occurrence_segments(indices, scores, lags, lengths, n):
    """Non-overlapping spans over ALL cells of one recording of n sub-fingerprints, from an occurrences call's matches (indices,
    scores and lags as Corpus.query_occurrences or decode_occurrence_keys give them; an index below 0 is no cell) and the
    sub-fingerprints of the entry each cell names.  Cell p spans [s, e) with s = max(0, -lag), e = min(n, -lag + length); cells
    with length 0, s >= n or e <= s are no candidates.  The candidates are visited in descending key order (higher score bits,
    then lower index), ties to the lower s, then the lower position p, and one is accepted when its span meets no accepted span
    (spans that only touch do not meet).  Returns (start int64[m], index int64[m], score float32[m], lag int32[m], length
    uint32[m]) sorted by start.  Unlike timeline_segments this sees every cell, so the second best entry at an offset is
    reported where the winner there loses to a better overlapping span."""
    idx = np.asarray(indices, dtype=np.int64).reshape(-1)
    sc = np.ascontiguousarray(np.asarray(scores, dtype=np.float32).reshape(-1))
    lg = np.asarray(lags).reshape(-1).astype(np.int64)
    ln = np.asarray(lengths).reshape(-1).astype(np.int64) & 0xFFFFFFFF
    n = int(n)
    s = np.maximum(0, -lg)
    e = np.minimum(n, -lg + ln)
    at = np.flatnonzero((idx >= 0) & (ln > 0) & (s < n) & (e > s))
    bits = sc.view(np.uint32).astype(np.int64)
    # (descending score bits, ascending index, ascending start, ascending position; lexsort's last key is the primary one)
    order = at[np.lexsort((at, s[at], idx[at], -bits[at]))]
    taken = np.zeros(max(n, 0), dtype=bool)
    kept = []
    for p in order:
        if taken[s[p]:e[p]].any():
            continue
        taken[s[p]:e[p]] = True
        kept.append(int(p))
    kept = np.asarray(sorted(kept, key=lambda p: s[p]), dtype=np.int64)
    return s[kept].astype(np.int64), idx[kept], sc[kept], lg[kept].astype(np.int32), ln[kept].astype(np.uint32)


def occurrence_segments_device(keys, lags, lengths, counts, n: int, capacity: int, starts_out=None, keys_out=None, lags_out=None,
                               lengths_out=None, counts_out=None, want_lags: bool = True, want_lengths: bool = True, stream=None):
    """LBAudioDetectiveOccurrenceSegmentsFromKeysDevice: occurrence_segments on the device, for the rows of an occurrences call --
    keys int64 / lags int32 / lengths int32 (Corpus.entry_lengths_from_keys_device of the keys), [slots] for one recording of n
    sub-fingerprints or [recordings, slots] for a batch (slots <= 8192, n <= 8192), and counts: the occurrences call's int64
    counts ([recordings] or one value), or None for every slot of a row (concatenated shards' rows) -> (starts int32, keys int64,
    lags int32 or None, lengths int32 or None, all [recordings, capacity], counts int32 [recordings]) on the device,
    asynchronously on `stream`; for 1-D input the rows themselves ([capacity], ..., a scalar tensor).  A row holds its recording's
    non-overlapping spans in start order, key, lag and length unchanged -- ids_from_keys_device, gather_keys_device,
    align_keys_device and remove_keys_device read the key block as it is -- zeros behind them; counts are the true numbers of
    spans, never cut at `capacity`.  want_lags=False / want_lengths=False (and no such output given) pass NULL: the other outputs
    are the same.  Decode with decode_occurrence_segments."""
    import torch
    if keys.dim() not in (1, 2) or tuple(lags.shape) != tuple(keys.shape) or tuple(lengths.shape) != tuple(keys.shape):
        raise ValueError("keys, lags and lengths must be 1-D or 2-D tensors of one shape")
    for x, kinds, what in ((keys, (torch.int64, getattr(torch, "uint64", torch.int64)), "keys (int64 or uint64)"),
                           (lags, (torch.int32,), "lags (int32)"),
                           (lengths, (torch.int32, getattr(torch, "uint32", torch.int32)), "lengths (int32 or uint32)")):
        if not (x.is_cuda and x.is_contiguous() and x.dtype in kinds):
            raise ValueError(f"{what} must be a contiguous device tensor")
    R, slots = (1, keys.shape[0]) if keys.dim() == 1 else (keys.shape[0], keys.shape[1])
    if counts is not None:
        if not (counts.is_cuda and counts.is_contiguous() and counts.dtype in (torch.int64, getattr(torch, "uint64", torch.int64))
                and counts.numel() >= R):
            raise ValueError("counts must be a contiguous int64 device tensor with one value per recording")
    cap = int(capacity)
    if (starts_out is None or keys_out is None or counts_out is None or (want_lags and lags_out is None)
            or (want_lengths and lengths_out is None)):
        with torch.cuda.stream(stream):                 # (the blocks belong to the stream that fills them)
            shape = (max(1, R), max(1, cap))
            if starts_out is None:
                starts_out = torch.empty(shape, dtype=torch.int32, device=keys.device)
            if keys_out is None:
                keys_out = torch.empty(shape, dtype=torch.int64, device=keys.device)
            if want_lags and lags_out is None:
                lags_out = torch.empty(shape, dtype=torch.int32, device=keys.device)
            if want_lengths and lengths_out is None:
                lengths_out = torch.empty(shape, dtype=torch.int32, device=keys.device)
            if counts_out is None:
                counts_out = torch.empty(max(1, R), dtype=torch.int32, device=keys.device)
    _out_ok(starts_out, R * cap, "starts_out")
    _out_ok(keys_out, R * cap, "keys_out")
    _out_ok(counts_out, R, "counts_out")
    for x, what in ((lags_out, "lags_out"), (lengths_out, "lengths_out")):
        if x is not None:
            _out_ok(x, R * cap, what)
    _check(N.lib().LBAudioDetectiveOccurrenceSegmentsFromKeysDevice(
        _dev_ptr(keys), _dev_ptr(lags), _dev_ptr(lengths), _dev_ptr(counts) if counts is not None else None, R, slots, int(n), cap,
        _dev_ptr(starts_out), _dev_ptr(keys_out), _dev_ptr(lags_out) if lags_out is not None else None,
        _dev_ptr(lengths_out) if lengths_out is not None else None, _dev_ptr(counts_out), _stream_ptr(stream)),
        "OccurrenceSegmentsFromKeysDevice")
    if keys.dim() == 1:                                  # (outputs given as [capacity] or [1, capacity]: the row either way)
        def row(x):
            return x.reshape(-1)[:cap] if hasattr(x, "reshape") else x
        return (row(starts_out), row(keys_out), (row(lags_out) if lags_out is not None else None),
                (row(lengths_out) if lengths_out is not None else None),
                counts_out.reshape(-1)[0] if hasattr(counts_out, "reshape") else counts_out)
    return starts_out, keys_out, lags_out, lengths_out, counts_out


def decode_occurrence_segments(starts, keys, lags, lengths, counts, index_base: int = 0):
    """The rows of occurrence_segments_device on the host: per recording the (start int64[m], index int64[m], score float32[m],
    lag int32[m], length uint32[m]) arrays occurrence_segments returns, m = min(count, capacity), the index global minus
    index_base; a list with one tuple per recording, or the one tuple for 1-D rows.  Without lags or lengths that array is None."""
    def host(x, dtype):
        return np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x).astype(dtype)

    k = host(keys, np.int64).astype(np.uint64)
    one = k.ndim == 1
    k = k.reshape(1, -1) if one else k
    st = host(starts, np.int64).reshape(k.shape)
    lg = host(lags, np.int32).reshape(k.shape) if lags is not None else None
    ln = host(lengths, np.int64).astype(np.uint32).reshape(k.shape) if lengths is not None else None
    cnt = host(counts, np.int64).reshape(-1)
    out = []
    for r in range(k.shape[0]):
        m = min(int(cnt[r]), k.shape[1])
        idx = (0xFFFFFFFF - (k[r, :m] & np.uint64(0xFFFFFFFF))).astype(np.int64) - int(index_base)
        sc = (k[r, :m] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out.append((st[r, :m].copy(), idx, sc, lg[r, :m].copy() if lg is not None else None,
                    ln[r, :m].copy() if ln is not None else None))
    return out[0] if one else out


def decode_join_keys(keys, offsets, first: int = 0):
    """(rows int64[m], indices int64[m], scores float32[m], total) of a join's keys and CSR offsets (any int64 sequences):
    m = min(total, len(keys)), rows counted from `first` (the call's first row)."""
    k = np.asarray(keys.cpu().numpy() if hasattr(keys, "cpu") else keys, dtype=np.int64).astype(np.uint64).reshape(-1)
    off = np.asarray(offsets.cpu().numpy() if hasattr(offsets, "cpu") else offsets, dtype=np.int64).astype(np.uint64).reshape(-1)
    total = int(off[-1])
    k = k[:min(total, len(k))]
    rows = np.searchsorted(off, np.arange(len(k), dtype=np.uint64), side="right").astype(np.int64) - 1 + int(first)
    return (rows, (0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF))).astype(np.int64), (k >> np.uint64(32)).astype(np.uint32).view(np.float32),
            total)


def group_labels_from_keys_device(keys, n_entries: int, offsets=None, row_pitch: int = 0, first_row: int = 0, row_keys=None,
                                  index_base: int = 0, labels=None, reset: bool = True, stream=None, n_rows=None, n_slots=None,
                                  group_count=None):
    """LBAudioDetectiveGroupLabelsFromKeysDevice: the connected components of the graph whose edges are match keys on the device
    -> (labels int32 [n_entries], group_count int64 [1]), both on the device, asynchronously on `stream`.  labels[i] is the
    lowest entry index of i's component.  `keys` with `offsets` (int64 [rows + 1]) is a join's CSR; without offsets the keys
    are rows of row_pitch slots (a 2-d tensor gives its own pitch), the threshold batch calls' layout.  Row r is entry
    first_row + r, or the entry row_keys[r] names.  reset=False adds the edges to the grouping `labels` already holds.  n_rows
    and n_slots default to what the tensors hold; group_count may be given to be reused."""
    import torch
    assert keys.is_cuda and keys.is_contiguous() and keys.element_size() == 8
    if offsets is not None:
        assert offsets.is_cuda and offsets.is_contiguous() and offsets.element_size() == 8
        if n_rows is None:
            n_rows = offsets.numel() - 1
        _out_ok(offsets, n_rows + 1, "offsets")
        if n_slots is None:
            n_slots = keys.numel()
    else:
        if not row_pitch:
            if keys.dim() != 2:
                raise ValueError("pitched rows need row_pitch or a 2-d key tensor")
            row_pitch = keys.shape[1]
        if n_rows is None:
            n_rows = keys.numel() // row_pitch
        if n_slots is None:
            n_slots = n_rows * row_pitch
    _out_ok(keys, n_slots, "keys")
    if row_keys is not None:
        assert row_keys.is_cuda and row_keys.is_contiguous() and row_keys.element_size() == 8
        _out_ok(row_keys, n_rows, "row_keys")
    if labels is None:
        if not reset:
            raise ValueError("reset=False needs the labels of the calls before")
        labels = torch.empty(max(1, n_entries), dtype=torch.int32, device=keys.device)[:n_entries]
    assert labels.element_size() == 4
    _out_ok(labels, n_entries, "labels")
    if group_count is None:
        group_count = torch.empty(1, dtype=torch.int64, device=keys.device)
    _out_ok(group_count, 1, "group_count")
    _check(N.lib().LBAudioDetectiveGroupLabelsFromKeysDevice(_dev_ptr(keys) if n_slots else None, n_slots,
                                                             _dev_ptr(offsets) if offsets is not None else None, row_pitch, n_rows,
                                                             first_row, _dev_ptr(row_keys) if row_keys is not None else None,
                                                             index_base, n_entries, int(bool(reset)), _dev_ptr(labels),
                                                             _dev_ptr(group_count), _stream_ptr(stream)), "GroupLabelsFromKeysDevice")
    return labels, group_count


def group_extra_keys_from_labels_device(labels, capacity=None, index_base: int = 0, stream=None):
    """LBAudioDetectiveGroupExtraKeysFromLabelsDevice: the keys (score word 1.0f) of every entry whose label is not its own
    index -- everything except the first entry of each group -- in ascending index -> (keys int64 [capacity] on the device,
    0-padded, count): the true number, also above the capacity (None: one slot per entry).  Corpus.remove_keys_device and
    Corpus.gather_keys_device take the keys as they are.  Returns once the keys are written."""
    import torch
    assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 4
    n = labels.numel()
    if capacity is None:
        capacity = max(1, n)
    keys = torch.empty(max(1, capacity), dtype=torch.int64, device=labels.device)
    count = N.UInt64(0)
    _check(N.lib().LBAudioDetectiveGroupExtraKeysFromLabelsDevice(_dev_ptr(labels), n, index_base, capacity, _dev_ptr(keys),
                                                                  C.byref(count), _stream_ptr(stream)), "GroupExtraKeysFromLabelsDevice")
    return keys, int(count.value)


def synth_corpus_device(seed: int, first: int, n_entries: int, n_sub: int, subfp_len: int, out=None, stream=None):
    import torch
    if out is None:
        out = torch.empty((n_entries, n_sub, N.PACKED_BYTES), dtype=torch.uint8, device="cuda")
    _check(N.lib().LBAudioDetectiveSynthCorpusDevice(seed & 0xFFFFFFFF, first, n_entries, n_sub, subfp_len,
                                                     out.data_ptr(), _stream_ptr(stream)), "SynthCorpusDevice")
    return out
