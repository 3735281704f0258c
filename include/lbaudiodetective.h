/*
 * lbaudiodetective.h -- C ABI of the MI355X-native LBAudioDetective hot path.
 *
 * Part 1 re-declares, name for name and argument for argument, the public C interface of
 * the upstream library so that a caller of the reference links against
 * liblbaudiodetective.so unchanged.  Each declaration cites the upstream declaration it
 * replaces (D.h = LBAudioDetective/LBAudioDetective.h, Fp.h = LBAudioDetectiveFingerprint.h,
 * Fr.h = LBAudioDetectiveFrame.h).  Every function that computes (fingerprinting, Haar,
 * sign extraction, compare) runs HIP kernels on the current device; there is no CPU
 * fallback and the calls fail with kLBAudioDetectiveDeviceUnavailable when no GPU is usable.
 *
 * Part 2 adds what the reference lacks and a GPU needs: PCM-in entry points (Apple's
 * ExtAudioFile does not exist here), batch fingerprinting on device-resident clips, and a
 * device-resident reference-fingerprint corpus with a top-1 query that returns a key a
 * host can all-reduce (max) across GPUs.
 *
 * Threading: fingerprints, frames, streams and corpora are, like upstream's objects, not re-entrant -- one call at a
 * time per object; distinct objects are independent.  One process drives one GPU (the current HIP device at the time
 * of the call).  A DETECTIVE may be called from several threads and on several HIP streams (round 3): the frame-row
 * buffer between its two kernels, the kernels' claim counters, its conversion buffers and its timing events exist
 * once per detective, so the library serialises such calls -- a mutex around the host side of every entry point, and a
 * batch call that arrives on another stream than its predecessor first waits on the device (hipStreamWaitEvent) for
 * the predecessor's last kernel.  Results are correct; the calls do not overlap.  For overlap use one detective per
 * stream (they are cheap: a plan of a few tables).  Exception: while a stream is being captured into a hipGraph
 * nothing is recorded or awaited -- ordering replays against other work of the same detective is the caller's.
 *
 * Plain C, plain pointers and sizes only.  "Device pointer" means memory of the current
 * HIP device (e.g. torch.Tensor.data_ptr()); "stream" is a hipStream_t passed as void*
 * (NULL = the default stream).
 */
#ifndef LBAUDIODETECTIVE_H
#define LBAUDIODETECTIVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- MacTypes / CoreAudio types the upstream headers get from Apple's SDK ------------- */
#if !defined(__MACTYPES__) && !defined(LBAD_HAVE_MACTYPES)
typedef uint32_t UInt32;
typedef int32_t SInt32;
typedef uint64_t UInt64;
typedef int64_t SInt64;
typedef float Float32;
typedef double Float64;
typedef unsigned char Boolean;
typedef SInt32 OSStatus;
enum { noErr = 0 };
#endif

#if !defined(__CoreAudioTypes_h__) && !defined(LBAD_HAVE_COREAUDIOTYPES)
/* layout-compatible with CoreAudio's AudioStreamBasicDescription */
typedef struct AudioStreamBasicDescription {
    Float64 mSampleRate;
    UInt32 mFormatID;
    UInt32 mFormatFlags;
    UInt32 mBytesPerPacket;
    UInt32 mFramesPerPacket;
    UInt32 mBytesPerFrame;
    UInt32 mChannelsPerFrame;
    UInt32 mBitsPerChannel;
    UInt32 mReserved;
} AudioStreamBasicDescription;
enum {
    kAudioFormatLinearPCM = 0x6C70636D, /* 'lpcm' */
    kAudioFormatFlagIsFloat = 1u << 0,
    kAudioFormatFlagIsPacked = 1u << 3
};
#endif

/* Upstream's two file entry points take NSURL* (D.h:218,235).  The library itself is plain C and takes filesystem
 * paths: a C / C++ host calls LBAudioDetectiveProcessAudioURL / ...CompareAudioURLs with a `const char*` in the
 * NSURL's place; an Objective-C host keeps passing NSURL* -- in Objective-C mode the two names are inline
 * wrappers (below, after the declarations) that hand `[[url path] fileSystemRepresentation]` to the path-taking
 * symbols LBAudioDetectiveProcessAudioPath / ...CompareAudioPaths.  No Apple header is needed for that. */
#ifdef __OBJC__
@class NSURL;
typedef NSURL* LBAudioDetectiveURLRef;
#else
typedef const char* LBAudioDetectiveURLRef;
#endif

/* ---- constants (D.h:14-20; values LBAudioDetective.m:20-26) ---------------------------- */
extern const OSStatus kLBAudioDetectiveArgumentInvalid;           /* D.h:14  (= 1) */
extern const UInt32 kLBAudioDetectiveDefaultWindowSize;           /* D.h:16  (= 2048) */
extern const UInt32 kLBAudioDetectiveDefaultAnalysisStride;       /* D.h:17  (= 64) */
extern const UInt32 kLBAudioDetectiveDefaultNumberOfPitchSteps;   /* D.h:18  (= 32) */
extern const UInt32 kLBAudioDetectiveDefaultSubfingerprintLength; /* D.h:20  (= 200) */
/* additions: status codes of this implementation */
extern const OSStatus kLBAudioDetectiveDeviceUnavailable;         /* 'nogp' */
extern const OSStatus kLBAudioDetectiveDeviceError;               /* 'gper' */
extern const OSStatus kLBAudioDetectiveUnsupportedFile;           /* 'fmt?' */
extern const OSStatus kLBAudioDetectiveMemFull;                   /* -108 (MacErrors.h memFullErr): a host allocation failed */
extern const OSStatus kLBAudioDetectiveCollectiveError;           /* 'rccl': RCCL missing or a collective failed */

typedef struct LBAudioDetective* LBAudioDetectiveRef;                       /* D.h:22 */
typedef struct LBAudioDetectiveFingerprint* LBAudioDetectiveFingerprintRef; /* Fp.h:11 */
typedef struct LBAudioDetectiveFrame* LBAudioDetectiveFrameRef;             /* Fr.h:11 */

/* ======================================================================================
 * Part 1a -- detective (D.h)
 * ==================================================================================== */
LBAudioDetectiveRef LBAudioDetectiveNew(void);                                            /* D.h:41 */
OSStatus LBAudioDetectiveDispose(LBAudioDetectiveRef inDetective);                        /* D.h:49 */
AudioStreamBasicDescription LBAudioDetectiveDefaultProcessingFormat(void);                /* D.h:62 */
Float64 LBAudioDetectiveGetProcessingSampleRate(LBAudioDetectiveRef inDetective);         /* D.h:74 */
UInt32 LBAudioDetectiveGetNumberOfPitchSteps(LBAudioDetectiveRef inDetective);            /* D.h:85 */
UInt32 LBAudioDetectiveGetSubfingerprintLength(LBAudioDetectiveRef inDetective);          /* D.h:96,129 */
UInt32 LBAudioDetectiveGetWindowSize(LBAudioDetectiveRef inDetective);                    /* D.h:107 */
UInt32 LBAudioDetectiveGetAnalysisStride(LBAudioDetectiveRef inDetective);                /* D.h:118 */
OSStatus LBAudioDetectiveSetProcessingSampleRate(LBAudioDetectiveRef inDetective, Float64 inSampleRate);        /* D.h:154 */
OSStatus LBAudioDetectiveSetNumberOfPitchSteps(LBAudioDetectiveRef inDetective, UInt32 inNumberOfPitchSteps);   /* D.h:164 */
OSStatus LBAudioDetectiveSetSubfingerprintLength(LBAudioDetectiveRef inDetective, UInt32 inSubfingerprintLength); /* D.h:174,205 */
/* Unlike LBAudioDetective.m:185-187 (which reports an error for every valid size), this
 * returns noErr for a power of two in [16, 8192] and kLBAudioDetectiveArgumentInvalid,
 * leaving the detective unchanged, for anything else. */
OSStatus LBAudioDetectiveSetWindowSize(LBAudioDetectiveRef inDetective, UInt32 inWindowSize);       /* D.h:184 */
OSStatus LBAudioDetectiveSetAnalysisStride(LBAudioDetectiveRef inDetective, UInt32 inAnalysisStride); /* D.h:194 */
/* File front end replacing ExtAudioFile: CAF ('lpcm' or Apple 'ima4') and RIFF/WAVE (PCM, IEEE
 * float), channels averaged to mono, converted to the processing sample rate by a documented
 * windowed-sinc resampler (Apple's converter is closed source; the container is parsed on the host, payload
 * decode, conversion and everything after it run on the GPU), then fingerprinted.
 * Other payloads return kLBAudioDetectiveUnsupportedFile, a missing file -43 (fnfErr). */
OSStatus LBAudioDetectiveProcessAudioPath(LBAudioDetectiveRef inDetective, const char* inFilePath,
                                          LBAudioDetectiveFingerprintRef* outFingerprint);
OSStatus LBAudioDetectiveCompareAudioPaths(LBAudioDetectiveRef inDetective, const char* inFilePath1, const char* inFilePath2,
                                           UInt32 inComparisonRange, Float32* outMatch);
#ifndef __OBJC__
/* the same two functions under upstream's names (exported symbols; LBAudioDetectiveURLRef is const char* here) */
OSStatus LBAudioDetectiveProcessAudioURL(LBAudioDetectiveRef inDetective, LBAudioDetectiveURLRef inFileURL,
                                         LBAudioDetectiveFingerprintRef* outFingerprint); /* D.h:218 */
OSStatus LBAudioDetectiveCompareAudioURLs(LBAudioDetectiveRef inDetective, LBAudioDetectiveURLRef inFileURL1,
                                          LBAudioDetectiveURLRef inFileURL2, UInt32 inComparisonRange,
                                          Float32* outMatch);                             /* D.h:235 */
#endif

/* Addition: many files in one call -- upstream's tests fingerprint 200 files per test, one call each
 * (LBAudioDetectiveTests.m:57-91).  The files are read and parsed by a pool of up to 16 threads that the library starts
 * on the first batch of four or more files and keeps for the life of the process (shared by all detectives); decode,
 * conversion, the window loop and the Haar / sign stage of ALL files run as one launch chain (one per distinct hop when the files' sample rates
 * differ); the converted samples never leave the device.  outFingerprints[i] is what
 * LBAudioDetectiveProcessAudioURL returns for file i (NULL if it failed); outStatuses (optional) receives every
 * file's status, and the call then returns noErr whenever the batch itself could run; without it the first
 * failing file's status is returned.  LBAudioDetectiveProcessAudioURL / ...CompareAudioURLs are this call with
 * one / two files. */
OSStatus LBAudioDetectiveProcessAudioURLs(LBAudioDetectiveRef inDetective, const char* const* inFilePaths, UInt32 inCount,
                                          LBAudioDetectiveFingerprintRef* outFingerprints, OSStatus* outStatuses);
/* A call of many files runs as a two-slot pipeline (round 4): the files go through in runs (an eighth of the call's bytes,
 * at least 16 MB, at most 512 MB), the host reads and parses run i + 1 into a second pinned block while the device decodes,
 * converts and fingerprints run i, and unpacks run i's results while the device works on run i + 1.  Results do not
 * depend on it.  SetFilePipeline(detective, 0) makes the call take one run at a time again (measurement). */
OSStatus LBAudioDetectiveSetFilePipeline(LBAudioDetectiveRef inDetective, UInt32 inEnabled);
/* Parity aid: the file front end alone, on the device -- the mono samples at the processing rate that the window
 * loop of LBAudioDetectiveProcessAudioURL consumes (payload decode + conversion, k_decode.hip / k_resample.hip),
 * copied to a host buffer the caller releases with LBAudioDetectiveFreeSamples; outFileFrames = the file's length
 * in FILE frames (LBAudioDetective.m:236). */
OSStatus LBAudioDetectiveConvertAudioURL(LBAudioDetectiveRef inDetective, const char* inFilePath, Float32** outSamples,
                                         UInt64* outCount, UInt64* outFileFrames, Float64* outFileSampleRate);

/* ======================================================================================
 * Part 1b -- fingerprint (Fp.h).  Sub-fingerprints cross this API as unpacked Booleans.
 * ==================================================================================== */
LBAudioDetectiveFingerprintRef LBAudioDetectiveFingerprintNew(UInt32 inSubfingerprintLength);            /* Fp.h:27 */
void LBAudioDetectiveFingerprintDispose(LBAudioDetectiveFingerprintRef inFingerprint);                  /* Fp.h:35 */
LBAudioDetectiveFingerprintRef LBAudioDetectiveFingerprintCopy(LBAudioDetectiveFingerprintRef inFingerprint); /* Fp.h:45 */
UInt32 LBAudioDetectiveFingerprintGetSubfingerprintLength(LBAudioDetectiveFingerprintRef inFingerprint);  /* Fp.h:59 */
UInt32 LBAudioDetectiveFingerprintGetNumberOfSubfingerprints(LBAudioDetectiveFingerprintRef inFingerprint); /* Fp.h:70 */
UInt32 LBAudioDetectiveFingerprintGetSubfingerprintAtIndex(LBAudioDetectiveFingerprintRef inFingerprint, UInt32 inIndex,
                                                           Boolean* outSubfingerprint);               /* Fp.h:83 */
Boolean LBAudioDetectiveFingerprintSetSubfingerprintLength(LBAudioDetectiveFingerprintRef inFingerprint,
                                                           UInt32* ioSubfingerprintLength);           /* Fp.h:98 */
void LBAudioDetectiveFingerprintAddSubfingerprint(LBAudioDetectiveFingerprintRef inFingerprint,
                                                  Boolean* inSubfingerprint);                         /* Fp.h:108 */
Boolean LBAudioDetectiveFingerprintEqualToFingerprint(LBAudioDetectiveFingerprintRef inFingerprint1,
                                                      LBAudioDetectiveFingerprintRef inFingerprint2); /* Fp.h:122 */
/* GPU: XOR/popcount compare kernel; returns NaN if the device call fails. */
Float32 LBAudioDetectiveFingerprintCompareToFingerprint(LBAudioDetectiveFingerprintRef inFingerprint1,
                                                        LBAudioDetectiveFingerprintRef inFingerprint2,
                                                        UInt32 inRange);                              /* Fp.h:134 */
Float32 LBAudioDetectiveFingerprintCompareSubfingerprints(LBAudioDetectiveFingerprintRef inFingerprint,
                                                          Boolean* inSubfingerprint1, Boolean* inSubfingerprint2,
                                                          UInt32 inRange);                            /* Fp.h:147 */

/* Wire format of a fingerprint: '0'/'1' per Boolean, sub-fingerprints joined by '+' (the string the
 * upstream test helper builds, LBAudioDetectiveTests.m:22-37).  GetString writes a NUL-terminated
 * string when inCapacity suffices and always returns the length needed (without the NUL);
 * NewFromString returns NULL for malformed input. */
UInt64 LBAudioDetectiveFingerprintGetStringLength(LBAudioDetectiveFingerprintRef inFingerprint);
UInt64 LBAudioDetectiveFingerprintGetString(LBAudioDetectiveFingerprintRef inFingerprint, char* outString, UInt64 inCapacity);
LBAudioDetectiveFingerprintRef LBAudioDetectiveFingerprintNewFromString(const char* inString);

/* ======================================================================================
 * Part 1c -- frame (Fr.h; "internal" upstream but used by its Haar test)
 * ==================================================================================== */
LBAudioDetectiveFrameRef LBAudioDetectiveFrameNew(UInt32 inMaxRowCount);                       /* Fr.h:27 */
void LBAudioDetectiveFrameDispose(LBAudioDetectiveFrameRef inFrame);                           /* Fr.h:35 */
LBAudioDetectiveFrameRef LBAudioDetectiveFrameCopy(LBAudioDetectiveFrameRef inFrame);          /* Fr.h:45 */
UInt32 LBAudioDetectiveFrameGetNumberOfRows(LBAudioDetectiveFrameRef inFrame);                 /* Fr.h:59 */
Float32* LBAudioDetectiveFrameGetRow(LBAudioDetectiveFrameRef inFrame, UInt32 inRowIndex);     /* Fr.h:71 */
Float32 LBAudioDetectiveFrameGetValue(LBAudioDetectiveFrameRef inFrame, UInt32 inRowIndex, UInt32 inColumnIndex); /* Fr.h:83 */
Boolean LBAudioDetectiveFrameFull(LBAudioDetectiveFrameRef inFrame);                           /* Fr.h:93 */
Boolean LBAudioDetectiveFrameSetRow(LBAudioDetectiveFrameRef inFrame, Float32* inRow, UInt32 inRowIndex, UInt32 inCount); /* Fr.h:110 */
void LBAudioDetectiveFrameDecompose(LBAudioDetectiveFrameRef inFrame);                         /* Fr.h:121  (GPU Haar) */
size_t LBAudioDetectiveFrameFingerprintSize(LBAudioDetectiveFrameRef inFrame);                 /* Fr.h:131 */
UInt32 LBAudioDetectiveFrameFingerprintLength(LBAudioDetectiveFrameRef inFrame);               /* Fr.h:141 */
void LBAudioDetectiveFrameExtractFingerprint(LBAudioDetectiveFrameRef inFrame, UInt32 inNumberOfWavelets,
                                             Boolean* outFingerprint);                         /* Fr.h:151 (GPU rank) */
Boolean LBAudioDetectiveFrameEqualToFrame(LBAudioDetectiveFrameRef inFrame1, LBAudioDetectiveFrameRef inFrame2); /* Fr.h:162 */

/* ======================================================================================
 * Part 2 -- additions
 * ==================================================================================== */

/* How the file entry points walk a file whose rate differs from the processing rate.
 * Hop mode 1 (default) is what upstream does (LBAudioDetective.m:236,250,275,287-288): its
 * length and its seek offsets are in FILE frames while every read asks for windowSize frames at the
 * PROCESSING rate, so the window count is (fileFrames - windowSize) / analysisStride and the hop is
 * analysisStride * processingRate / fileRate processing-rate samples (rounded, at least 1).
 * Hop mode 0: analysisStride samples at the processing rate, like the PCM entry points. */
OSStatus LBAudioDetectiveSetFileHopMode(LBAudioDetectiveRef inDetective, UInt32 inMode);
/* NOTE on defaults: since round 2 the file entry points default to hop mode 1 and tail mode 1 (upstream's
 * behaviour; round 1 shipped hop mode 0 / zero-filled tails).  For a file whose rate differs from the processing
 * rate the two give different fingerprints, so a corpus built from FILES with the round-1 defaults must be
 * rebuilt, or queried with LBAudioDetectiveSetFileHopMode(d, 0).  Fingerprints of PCM are unaffected. */
/* Hop mode 1 only -- the windows upstream starts so close to the end of the file that ExtAudioFileRead
 * cannot deliver windowSize frames (the last ~windowSize * fileRate / processingRate file frames):
 *   1 (default) the read delivers nothing: inNumberFrames = 0 makes every band of the row 0.0
 *     (LBAudioDetective.m:382-383,404).  This is the behaviour that reproduces the essay's Fig. 24
 *     (eight lossless `_eql` fixtures within 0.5 points);
 *   2 partial reads, literally: the unread part of the in-place FFT buffer keeps the previous window's
 *     packed spectrum and nRead replaces the window size in the band arithmetic (:275,281,351-355,373-395);
 *   0 the unread part is cleared (not upstream). */
OSStatus LBAudioDetectiveSetFileTailMode(LBAudioDetectiveRef inDetective, UInt32 inMode);
/* Converter model of the file entry points (Apple's is closed source): 0 (default) Kaiser-windowed sinc,
 * 24 zero crossings, cut-off 0.92 Nyquist; 1 short sinc (4 zero crossings, cut-off at Nyquist: leaky);
 * 2 linear interpolation (no anti-alias filter). */
OSStatus LBAudioDetectiveSetResamplerMode(LBAudioDetectiveRef inDetective, UInt32 inMode);
/* Decode a file to mono float32, optionally converted to inSampleRate (0 = keep the file's rate): host code
 * (no detective, no device), the samples LBAudioDetectiveProcessAudioURL's device converter produces.
 * The buffer is owned by the caller and released with LBAudioDetectiveFreeSamples. */
OSStatus LBAudioDetectiveReadAudioURL(const char* inFilePath, Float64 inSampleRate, Float32** outSamples,
                                      UInt64* outCount, Float64* outSampleRate);
OSStatus LBAudioDetectiveReadAudioURLWithResampler(const char* inFilePath, Float64 inSampleRate,
                                                   UInt32 inResamplerMode, Float32** outSamples, UInt64* outCount,
                                                   Float64* outSampleRate);
void LBAudioDetectiveFreeSamples(Float32* inSamples);
/* The file loop of LBAudioDetective.m:241-293 on a file that is already decoded and converted:
 * inClientSamples = the whole file at the processing rate, inFileFrames = its length in FILE frames (what
 * kExtAudioFileProperty_FileLengthFrames reports, :236), inHop = processing-rate samples between window
 * starts.  Honours the file tail mode.  LBAudioDetectiveProcessAudioURL in hop mode 1 is
 * decode + convert + this. */
OSStatus LBAudioDetectiveProcessFileStream(LBAudioDetectiveRef inDetective, const Float32* inClientSamples,
                                           UInt64 inClientCount, UInt64 inFileFrames, UInt32 inHop,
                                           LBAudioDetectiveFingerprintRef* outFingerprint);

/* Number of sub-fingerprints a buffer of inNumberOfSamples yields with the detective's
 * window/stride (framing of LBAudioDetective.m:250-255; 0 when shorter than a window). */
UInt64 LBAudioDetectiveGetSubfingerprintCount(LBAudioDetectiveRef inDetective, UInt64 inNumberOfSamples);

/* Replaces the ExtAudioFile loop of LBAudioDetective.m:224-290: host float32 mono PCM that
 * is already at the processing sample rate -> fingerprint. */
OSStatus LBAudioDetectiveProcessPCM(LBAudioDetectiveRef inDetective, const Float32* inSamples,
                                    UInt64 inNumberOfSamples, LBAudioDetectiveFingerprintRef* outFingerprint);
/* LBAudioDetectiveCompareAudioURLs (LBAudioDetective.m:442-464) on two PCM buffers. */
OSStatus LBAudioDetectiveComparePCM(LBAudioDetectiveRef inDetective, const Float32* inSamples1, UInt64 inCount1,
                                    const Float32* inSamples2, UInt64 inCount2, UInt32 inComparisonRange,
                                    Float32* outMatch);

/* Packed sub-fingerprint: LBAD_PACKED_WORDS little-endian 32-bit words; Boolean b of the
 * sub-fingerprint is bit (b & 31) of word (b >> 5); unused high bits are zero.  The device
 * path supports subfingerprintLength <= 256. */
#define LBAD_PACKED_WORDS 8
#define LBAD_PACKED_BYTES 32
#define LBAD_MAX_SUBFINGERPRINT_LENGTH 256

/* Batch hot path: inClips = device pointer to inNumberOfClips x inSamplesPerClip float32,
 * outPacked = device pointer to inNumberOfClips x count x LBAD_PACKED_BYTES, where
 * count = LBAudioDetectiveGetSubfingerprintCount(d, inSamplesPerClip).  Asynchronous on
 * inStream. */
OSStatus LBAudioDetectiveFingerprintClipsDevice(LBAudioDetectiveRef inDetective, const Float32* inClips,
                                                UInt64 inNumberOfClips, UInt64 inSamplesPerClip,
                                                void* outPacked, void* inStream);
/* Same with integer PCM: inSampleFormat 0 = float32, 1 = int16 (sample / 32768), 2 = int32
 * (sample / 2^31).  The conversion LBAudioDetectiveConvertToFormat (LBAudioDetective.m:413-437) hands
 * to AudioConverter is fused into the kernels' PCM load; int16 input halves the HBM read traffic. */
OSStatus LBAudioDetectiveFingerprintClipsDeviceFormat(LBAudioDetectiveRef inDetective, const void* inClips,
                                                      UInt32 inSampleFormat, UInt64 inNumberOfClips,
                                                      UInt64 inSamplesPerClip, void* outPacked, void* inStream);
/* Same, host buffers in and unpacked Booleans out (count x subfingerprintLength per clip). */
OSStatus LBAudioDetectiveFingerprintClips(LBAudioDetectiveRef inDetective, const Float32* inClips,
                                          UInt64 inNumberOfClips, UInt64 inSamplesPerClip, Boolean* outBooleans);
/* Same with integer PCM in host memory (inSampleFormat as above): int16 halves the bytes that cross
 * PCIe, which is what bounds this entry point. */
OSStatus LBAudioDetectiveFingerprintClipsFormat(LBAudioDetectiveRef inDetective, const void* inClips,
                                                UInt32 inSampleFormat, UInt64 inNumberOfClips,
                                                UInt64 inSamplesPerClip, Boolean* outBooleans);
/* Frame phases.  A sub-fingerprint is one frame of 128 rows, and a clip's frame grid starts at its first sample; a
 * recording that starts anywhere else shares no frame with it.  inPhases (P: 1, 2, 4, 8, 16 or 32) grids, h = 128 / P rows
 * apart: phase p of a signal x[0, L) is the signal x[p * h * stride, L), and its sub-fingerprints are those of
 * LBAudioDetectiveProcessPCM on that signal, bit for bit.  Their number: 0 when L is shorter than the offset, else
 * LBAudioDetectiveGetSubfingerprintCount(d, L - p * h * stride) -- count_0 or count_0 - 1.  0 for a P outside the six values
 * or inPhase >= inPhases. */
UInt64 LBAudioDetectiveGetSubfingerprintCountAtPhase(LBAudioDetectiveRef inDetective, UInt64 inNumberOfSamples, UInt32 inPhases,
                                                     UInt32 inPhase);
/* The batch call at inPhases phases: outPacked = DEVICE, [inNumberOfClips][inPhases][count_0] x LBAD_PACKED_BYTES with
 * count_0 = LBAudioDetectiveGetSubfingerprintCount(d, inSamplesPerClip); the slots at and behind a phase's count are zero.
 * The windows of a clip are transformed ONCE (stage 1 as in the batch call, plus at most one frame of rows per clip for the
 * phases' last frames), stage 2 runs per (phase, frame) with frames at a row hop.  inSampleFormat as above; asynchronous on
 * inStream; walks the clips in chunks under LBAudioDetectiveSetScratchLimit.  inPhases == 1 writes what
 * LBAudioDetectiveFingerprintClipsDeviceFormat writes.  kLBAudioDetectiveArgumentInvalid for another P. */
OSStatus LBAudioDetectiveFingerprintClipsDevicePhases(LBAudioDetectiveRef inDetective, const void* inClips, UInt32 inSampleFormat,
                                                      UInt64 inNumberOfClips, UInt64 inSamplesPerClip, UInt32 inPhases,
                                                      void* outPacked, void* inStream);
/* Kernel selection for the batch path: 0 = automatic, 1 = generic kernels (any window size / band count / stride),
 * 2 = specialised kernels only -- ArgumentInvalid when the configuration has no specialised stage-1 kernel:
 *   - stride 64: pruned 1024-point FFT for bands that read only bins 0..21; streaming 2048- / 4096-point kernels that
 *     share the early FFT stages between consecutive windows (clips that start on 8-byte boundaries: an even clip
 *     length or a single clip; <= 32 bands);
 *   - register-resident FFT of 256- to 2048-sample windows for any band table at ANY EVEN stride (float32 input when
 *     the stride is not 64; the span of a workgroup's windows must fit the LDS budget) -- among them the hop of 8
 *     samples the file entry points use for 44.1 kHz material at the defaults;
 *   - register Haar / select for frames of 16, 32 or 64 bands.
 * 3 = like 2 but the register-resident 2048-point kernel instead of the streaming one (measurement). */
OSStatus LBAudioDetectiveSetKernelVariant(LBAudioDetectiveRef inDetective, UInt32 inVariant);
/* How the pruned stage 1 (k_rows_pruned.hip) adds a band's power terms: 0 = automatic, 1 = through LDS
 * (frame_rows_pruned_kernel, any table the pruned kernel accepts), 2 = in the lanes that computed them
 * (frame_rows_lanes_kernel: the default 44.1 kHz / 1024 / 32-band table at stride 64) -- ArgumentInvalid where the present
 * settings do not have that form.  Automatic takes form 2 where it exists.  Results never depend on it.
 * LBAudioDetectiveGetBandSumForm: the form (1 or 2) a call under the present settings would take; it reads the settings, no
 * device.  Form 2 that was set under other settings is checked again by every call: where the settings have lost the form,
 * the getter says 1 and the batch call returns ArgumentInvalid until the form is set anew. */
OSStatus LBAudioDetectiveSetBandSumForm(LBAudioDetectiveRef inDetective, UInt32 inForm);
OSStatus LBAudioDetectiveGetBandSumForm(LBAudioDetectiveRef inDetective, UInt32* outForm);
/* Measurement knobs of the generic stage-1 kernel (the LDS-tile sizing sweep of tools/sweep_lds_tiles.py):
 * waves per workgroup (0 = automatic; a value the window size has no instance for, or that does not fit the LDS with the
 * cache as asked, falls back to the smallest workgroup without the cache) and whether the shared per-lane twiddle cache is
 * used (default 1).  Results never depend on them; LBAudioDetectiveDebugStage1Choice tells which instance a setting takes. */
OSStatus LBAudioDetectiveSetKernelTuning(LBAudioDetectiveRef inDetective, UInt32 inWavesPerWorkgroup,
                                         UInt32 inTwiddleCache);
/* HBM the frame-row buffer between the two kernels may take (default 512 MiB; 16 KiB per frame at 32
 * bands).  Batches that need more are processed in several launches. */
OSStatus LBAudioDetectiveSetScratchLimit(LBAudioDetectiveRef inDetective, UInt64 inBytes);
/* Measurement aid: once enabled, every batch call records HIP events on its stream around the two
 * kernels; GetStageTimes waits for the last batch and returns, summed over all batch calls since
 * timing was (re-)enabled, the durations (ms) of stage 1 (windows -> frame rows) and stage 2
 * (Haar + select) and the number of launches of each. */
OSStatus LBAudioDetectiveSetStageTiming(LBAudioDetectiveRef inDetective, UInt32 inEnabled);
OSStatus LBAudioDetectiveGetStageTimes(LBAudioDetectiveRef inDetective, Float32* outStage1Ms, Float32* outStage2Ms,
                                       UInt32* outLaunches);
/* Debug taps for stage-level parity tests: device buffers of
 * clips x count x 128 x bands float32 receiving the frame before / after the Haar; either may be NULL. */
OSStatus LBAudioDetectiveFingerprintClipsDeviceTaps(LBAudioDetectiveRef inDetective, const Float32* inClips,
                                                    UInt64 inNumberOfClips, UInt64 inSamplesPerClip,
                                                    void* outPacked, Float32* outFramesRaw, Float32* outFramesHaar,
                                                    void* inStream);
/* The same with integer PCM (inSampleFormat as in LBAudioDetectiveFingerprintClipsDeviceFormat): the frame rows every
 * stage-1 kernel makes of int16 / int32 samples, for comparison with the reference's.  A raw tap keeps full rows between the
 * stages (no compact frames). */
OSStatus LBAudioDetectiveFingerprintClipsDeviceTapsFormat(LBAudioDetectiveRef inDetective, const void* inClips,
                                                          UInt32 inSampleFormat, UInt64 inNumberOfClips,
                                                          UInt64 inSamplesPerClip, void* outPacked, Float32* outFramesRaw,
                                                          Float32* outFramesHaar, void* inStream);
/* Debug / tests: which kernels ONE batch call (LBAudioDetectiveFingerprintClipsDevice and its kin) takes -- the call's own
 * decision (api_detective.cpp: stage1_choose, and the instance functions of the kernel files that the launchers dispatch on)
 * as words; touches no device.  The call is described by the settings, the kernel variant, the tuning
 * (LBAudioDetectiveSetKernelTuning's two values), the sample format, the number of clips and samples per clip, the clip
 * pointer's address modulo 8, whether the raw tap is wanted and whether a file tail is attached (the file entry points).
 * Returns kLBAudioDetectiveArgumentInvalid for a NULL outWords, inCapacity < 12, a variant above 4, more than 16 waves or an
 * address above 7; otherwise noErr and outWords:
 *   0 the status the call would return on a working device (an OSStatus as UInt32)   1 whether kernels are launched (0: the
 *   status is an error, or there is no clip or no whole frame -- every later word is 0)   2 the stage-1 family: 0
 *   fft_bands_kernel (generic), 1 frame_rows_pruned_kernel, 2 rows_stream2_kernel, 3 rows_full_kernel, 4 rows_stream_kernel
 *   3..6 the instance's template arguments: LOG2W, WPB, CACHED | FMT | FMT, QLO, QHI | LOG2L, FMT, S64, lean (SKIP != 0) | FMT
 *   (the generic kernel reads the sample format at run time)   7 rows between the stages: 0 full, 1 compact   8 stage 2: 0
 *   haar_select_kernel (generic), 1 k_haar_select32.hip, 2 its sparse form   9 the waves asked for were not taken   10 the
 *   twiddle cache asked for was not taken (9 or 10 set: the tuning fell back)   11 frames per clip */
OSStatus LBAudioDetectiveDebugStage1Choice(Float64 inSampleRate, UInt32 inWindowSize, UInt32 inAnalysisStride,
                                           UInt32 inNumberOfPitchSteps, UInt32 inSubfingerprintLength, UInt32 inKernelVariant,
                                           UInt32 inWavesPerWorkgroup, UInt32 inTwiddleCache, UInt32 inSampleFormat,
                                           UInt64 inNumberOfClips, UInt64 inSamplesPerClip, UInt32 inClipAddressMod8,
                                           UInt32 inRawTap, UInt32 inFileTail, UInt32* outWords, UInt32 inCapacity);

/* Streaming (the essay's live-recording use): PCM arrives in chunks of any size; whenever the
 * buffered samples complete one or more frames they are fingerprinted and appended, and the partial
 * frame is carried to the next call.  After pushing L samples in total the fingerprint equals
 * LBAudioDetectiveProcessPCM on those L samples.  The detective's settings must not change while a
 * stream is open. */
typedef struct LBAudioDetectiveStream* LBAudioDetectiveStreamRef;
LBAudioDetectiveStreamRef LBAudioDetectiveStreamNew(LBAudioDetectiveRef inDetective);
void LBAudioDetectiveStreamDispose(LBAudioDetectiveStreamRef inStream);
OSStatus LBAudioDetectiveStreamPush(LBAudioDetectiveStreamRef inStream, const Float32* inSamples,
                                    UInt64 inNumberOfSamples, UInt32* outNewSubfingerprints);
LBAudioDetectiveFingerprintRef LBAudioDetectiveStreamCopyFingerprint(LBAudioDetectiveStreamRef inStream);

/* Stream bank: the same for MANY live channels at once, on the device.  A bank owns, in device memory, the carried partial frame
 * of each of its channels and each channel's inHistorySubfingerprints most recent sub-fingerprints (a ring) in the packed layout
 * (LBAD_PACKED_BYTES each) that every ...Packed...Device call reads.  One push takes a ragged block of new samples, fingerprints
 * every frame that became complete -- all channels in one launch chain -- and files the results.  After a channel has received L
 * samples in any chunking its sub-fingerprints are those of LBAudioDetectiveProcessPCM on the L samples, bit for bit.
 *
 * The bank takes window, stride, pitch steps and sub-fingerprint length from the detective when it is made; a push after any of
 * them changed returns kLBAudioDetectiveArgumentInvalid.  inFramesPerPass bounds the staging memory (that many frames of window +
 * 128 x stride samples; 0: one frame per channel): a push that completes more frames runs in several passes, with the same
 * results.  New returns NULL for a NULL detective, zero channels (more than 2^24), zero history (more than 2^20), without a device
 * or without memory; per channel the bank holds 2 x (window + 128 x stride) samples and 32 x history bytes.
 *
 * The sample counts are HOST memory, and the bank mirrors on the host what every channel carries and has produced: neither
 * PushDevice nor WindowDevice reads anything back, both are asynchronous on inStream.  A mutex guards the host side; a call on
 * another stream than the call before it first waits ON THE DEVICE for that call's last launch, so calls take effect in the order
 * they were made.  Argument checks that need no handle come first (NULL handles and required pointers, inSamples off 4 bytes,
 * outNewPacked / outPacked off 16 bytes), then kLBAudioDetectiveDeviceUnavailable without a device, then the rest -- a channel
 * index out of range, inNewCapacity below the push's total where outNewPacked is given, a window longer than the history or than
 * a listed channel's total -- each kLBAudioDetectiveArgumentInvalid; a refused call changes neither the mirror nor device memory.
 * A HIP failure behind a call's first launch leaves the device state unknown: the bank is unusable from then on, and every later
 * call returns kLBAudioDetectiveDeviceError (CopyFingerprint: NULL); only Dispose remains. */
typedef struct LBAudioDetectiveStreamBank* LBAudioDetectiveStreamBankRef;
LBAudioDetectiveStreamBankRef LBAudioDetectiveStreamBankNew(LBAudioDetectiveRef inDetective, UInt32 inNumberOfChannels,
                                                            UInt32 inHistorySubfingerprints, UInt32 inFramesPerPass);
/* A PHASED bank: the same at inPhases (1, 2, 4, 8, 16 or 32) frame phases (LBAudioDetectiveGetSubfingerprintCountAtPhase).  Its N
 * channels present N x inPhases VIRTUAL channels, v = c x inPhases + p: after channel c has received L samples in any chunking,
 * virtual channel v holds the sub-fingerprints of phase p of those L samples, bit for bit.  Every window of a channel is
 * transformed once, whatever inPhases: per channel the bank keeps the carried samples and a ring of its last 128 frame rows, a
 * push transforms the new windows (in groups of four rows, a group as soon as its last window is there) and runs stage 2 at a
 * row hop on every (channel, phase) frame they complete.  Which call takes which index: PushDevice / Push take N sample counts
 * and ResetChannels real channels (all phases of each start again); outNewCounts has N x inPhases entries and outNewPacked is
 * in virtual-channel order, then time order; GetCounts' totals have N x inPhases entries, its pending samples N; WindowDevice
 * and CopyFingerprint take virtual channel indices -- so every ...Packed...Device query runs on a phased bank's windows as it
 * is.  inFramesPerPass bounds the frames of one stage-2 launch and (x 128 rows) the windows staged for one stage-1 launch; 0: N x
 * inPhases.  It does NOT bound a push's memory as it does in the unphased bank: the rows a push transforms are kept for the whole
 * push (stage 2 reads them at every phase), one block of new windows x pitch steps x 4 bytes that grows to the largest push and
 * stays -- 88 KB per channel for one second at 44.1 kHz / stride 64 / 32 pitch steps.  NULL as LBAudioDetectiveStreamBankNew,
 * and for another inPhases, N x inPhases above 2^24 or a stride above the window.  Beside that block the bank holds, per channel,
 * the unphased bank's samples, 128 x pitch steps x 4 bytes of rows and 32 x history x inPhases bytes. */
LBAudioDetectiveStreamBankRef LBAudioDetectiveStreamBankNewPhased(LBAudioDetectiveRef inDetective, UInt32 inNumberOfChannels,
                                                                  UInt32 inHistorySubfingerprints, UInt32 inFramesPerPass,
                                                                  UInt32 inPhases);
UInt32 LBAudioDetectiveStreamBankGetPhases(LBAudioDetectiveStreamBankRef inBank);   /* 1 for an unphased bank, 0 for NULL */
/* host mirror of a phased bank's work since creation: windows transformed by stage 1 and frames selected by stage 2, over all
 * channels (either pointer may be NULL, not both); kLBAudioDetectiveArgumentInvalid for an unphased bank */
OSStatus LBAudioDetectiveStreamBankGetWork(LBAudioDetectiveStreamBankRef inBank, UInt64* outWindowsTransformed, UInt64* outFramesSelected);
void LBAudioDetectiveStreamBankDispose(LBAudioDetectiveStreamBankRef inBank);   /* waits for the bank's launches */
/* inSamples: DEVICE float32, the channels' new samples one after the other in channel order (4-byte aligned; a channel's run may
 * start at any sample; they are read until the call's launches have run).  inSampleCounts: HOST, one count per channel, 0 =
 * nothing for this channel.  outNewCounts (HOST, may be NULL): sub-fingerprints each channel completed in this call -- known when
 * the call returns.  outNewPacked (DEVICE, 16-byte aligned, may be NULL): those sub-fingerprints, 32 bytes each, in channel order
 * then in time order, written asynchronously on inStream; outNewTotal (may be NULL) their number.  A push that completes more
 * than the history's frames of a channel keeps the last of them there; all of them appear in outNewPacked and in the totals. */
OSStatus LBAudioDetectiveStreamBankPushDevice(LBAudioDetectiveStreamBankRef inBank, const Float32* inSamples,
                                              const UInt32* inSampleCounts, UInt32* outNewCounts, void* outNewPacked,
                                              UInt64 inNewCapacity, UInt64* outNewTotal, void* inStream);
/* the same with HOST samples; returns once inSamples may be reused; the outputs as above */
OSStatus LBAudioDetectiveStreamBankPush(LBAudioDetectiveStreamBankRef inBank, const Float32* inSamples,
                                        const UInt32* inSampleCounts, UInt32* outNewCounts, void* outNewPacked,
                                        UInt64 inNewCapacity, UInt64* outNewTotal, void* inStream);
/* host mirror, no device work: per channel the sub-fingerprints since creation / the last reset, and the samples carried (either
 * pointer may be NULL, not both) */
OSStatus LBAudioDetectiveStreamBankGetCounts(LBAudioDetectiveStreamBankRef inBank, UInt64* outTotals, UInt32* outPendingSamples);
/* the inSubfingerprints (>= 1) most recent sub-fingerprints of each listed channel, oldest first: outPacked = DEVICE
 * [inNumberOfChannels][inSubfingerprints][32 bytes], asynchronous on inStream.  inChannels: HOST; a channel may be listed more
 * than once, in any order; at most 2^31 sub-fingerprints per call. */
OSStatus LBAudioDetectiveStreamBankWindowDevice(LBAudioDetectiveStreamBankRef inBank, const UInt32* inChannels,
                                                UInt32 inNumberOfChannels, UInt32 inSubfingerprints, void* outPacked, void* inStream);
/* the min(total, history) most recent sub-fingerprints of one channel as a handle, oldest first (waits for the device) */
LBAudioDetectiveFingerprintRef LBAudioDetectiveStreamBankCopyFingerprint(LBAudioDetectiveStreamBankRef inBank, UInt32 inChannel);
/* the listed channels start again: nothing carried, total 0, empty history */
OSStatus LBAudioDetectiveStreamBankResetChannels(LBAudioDetectiveStreamBankRef inBank, const UInt32* inChannels, UInt32 inNumberOfChannels);
/* Debug / tests: the host plan of one push, needs no device.  Per channel, from inPending samples carried (below window + 128 x
 * stride) and inSampleCounts new ones: outReady = LBAudioDetectiveGetSubfingerprintCount's value for their sum, outPendingAfter =
 * the sum - outReady x 128 x stride, outKept = min(outReady, inHistorySubfingerprints), the frames the ring keeps. */
OSStatus LBAudioDetectiveDebugStreamBankPlan(UInt32 inWindowSize, UInt32 inAnalysisStride, UInt32 inHistorySubfingerprints,
                                             UInt32 inNumberOfChannels, const UInt32* inPending, const UInt32* inSampleCounts,
                                             UInt32* outReady, UInt32* outPendingAfter, UInt32* outKept);

/* Resampler bank: the sample-rate converter of the file front end in streaming form, for MANY live channels at once, on the
 * device -- what stands between live feeds (44.1 or 48 kHz, often int16) and a stream bank at the processing rate.  A bank owns,
 * in device memory, each channel's filter history and a copy of the rate pair's phase table.  One push takes a ragged block of new
 * samples and emits every output sample that became final -- all channels in one launch chain -- in the layout
 * LBAudioDetectiveStreamBankPushDevice reads: a resampler push followed by a stream-bank push of (outSamples, outNewCounts) on the
 * same stream is the whole path, with nothing read back.
 *
 * The arithmetic is the rational position of LBAudioDetectiveReadAudioURLWithResampler.  With inInputSampleRate /
 * inOutputSampleRate = p / q in lowest terms, output n of a channel sits at ip = (n p) div q with phase (n p) mod q and sums its
 * phase's taps x[ip + m]; m_lo / m_hi are the smallest first / largest last tap over the phases (-192 / 193 for 44100 -> 5512 Hz,
 * mode 0).  An output is final once its last possible tap has arrived: after a channel has received L samples since it started,
 * in any chunking, it has emitted emitted(L) = 0 for L <= m_hi, else ceil((L - m_hi) q / p) samples, and they are the first
 * emitted(L) samples the whole-signal converter gives for x[0, L') for every L' >= L long enough to have them, bit for bit.
 * Finishing a channel at L emits the outputs [emitted(L), n_out(L)), n_out(L) = (UInt64)(L / (rate_in / rate_out)), with taps at
 * or beyond L contributing nothing: the channel's whole output is then the whole-signal conversion of x[0, L) exactly, and the
 * channel starts again.
 *
 * New returns NULL for equal rates (push those samples straight into the stream bank), for a pair the rational position does not
 * cover (rates that are not whole numbers of Hz, q > 16384, p > 2^24, a ratio outside [1/4096, 4096]), for a mode other than 0
 * (long Kaiser sinc) or 1 (short sinc), for a pair whose tap span m_hi - m_lo + 1 exceeds LBAD_RESAMPLER_BANK_MAX_TAP_SPAN input
 * samples -- what a workgroup can stage; mode 0: a ratio above about 53, mode 1: above about 319 --, for zero or more than 2^24
 * channels, without a device or without memory.  Per channel the bank holds 2 x tap span samples.  It depends on no detective.
 *
 * The sample counts are HOST memory, and the bank mirrors on the host each channel's input total, output total and carried-buffer
 * side: no call reads anything back, PushDevice and FinishChannels are asynchronous on inStream.  A mutex guards the host side; a
 * call on another stream than the call before it first waits ON THE DEVICE for that call's last launch.  Argument checks that need
 * no handle come first (NULL handles and required pointers, inSampleFormat above 1, inSamples off 4 bytes (float32) / 2 bytes
 * (int16), outSamples off 4 bytes), then kLBAudioDetectiveDeviceUnavailable without a device, then the rest -- a channel index out
 * of range or listed twice, new samples without inSamples, outputs without outSamples, inCapacity below the call's total, more
 * than 2^31 - 1 outputs in one call, a channel whose n p would leave 63 bits -- each kLBAudioDetectiveArgumentInvalid; a refused
 * call changes neither the mirror nor device memory.  A HIP failure behind a call's first launch leaves the device state unknown:
 * every later call returns kLBAudioDetectiveDeviceError; only Dispose remains. */
#define LBAD_RESAMPLER_BANK_MAX_TAP_SPAN 2560
typedef struct LBAudioDetectiveResamplerBank* LBAudioDetectiveResamplerBankRef;
LBAudioDetectiveResamplerBankRef LBAudioDetectiveResamplerBankNew(Float64 inInputSampleRate, Float64 inOutputSampleRate,
                                                                  UInt32 inResamplerMode, UInt32 inNumberOfChannels);
void LBAudioDetectiveResamplerBankDispose(LBAudioDetectiveResamplerBankRef inBank);   /* waits for the bank's launches */
/* inSamples: DEVICE, the channels' new samples one after the other in channel order, exactly as StreamBankPushDevice takes them;
 * inSampleFormat 0: float32, 1: int16, read as (float)s * (1.0f / 32768.0f); a channel's run may start at any sample; they are
 * read until the call's launches have run.  inSampleCounts: HOST, one count per channel, 0 = nothing for this channel.
 * outNewCounts (HOST, may be NULL): one entry per channel of the bank, zeros included: the samples each channel emitted in this
 * call -- known when the call returns.  outSamples (DEVICE float32, 4-byte aligned): those samples in channel order, then in time
 * order, written asynchronously on inStream; inCapacity: its room in samples; outNewTotal (may be NULL): their number. */
OSStatus LBAudioDetectiveResamplerBankPushDevice(LBAudioDetectiveResamplerBankRef inBank, const void* inSamples, UInt32 inSampleFormat,
                                                 const UInt32* inSampleCounts, UInt32* outNewCounts, Float32* outSamples,
                                                 UInt64 inCapacity, UInt64* outNewTotal, void* inStream);
/* the same with HOST samples; returns once inSamples may be reused; the outputs as above */
OSStatus LBAudioDetectiveResamplerBankPush(LBAudioDetectiveResamplerBankRef inBank, const void* inSamples, UInt32 inSampleFormat,
                                           const UInt32* inSampleCounts, UInt32* outNewCounts, Float32* outSamples,
                                           UInt64 inCapacity, UInt64* outNewTotal, void* inStream);
/* the listed channels (HOST, each at most once) end their signals where they are: the outputs the whole-signal converter still
 * has for them, laid out and reported as a push's (channel order, whatever the list's), and the channels start again */
OSStatus LBAudioDetectiveResamplerBankFinishChannels(LBAudioDetectiveResamplerBankRef inBank, const UInt32* inChannels, UInt32 inNumberOfChannels,
                                                     UInt32* outNewCounts, Float32* outSamples, UInt64 inCapacity, UInt64* outNewTotal, void* inStream);
/* host mirror, no device work: per channel the samples received and emitted since it (re)started (either pointer may be NULL,
 * not both) */
OSStatus LBAudioDetectiveResamplerBankGetCounts(LBAudioDetectiveResamplerBankRef inBank, UInt64* outInputTotals, UInt64* outOutputTotals);
/* the listed channels start again without emitting anything: totals 0, nothing carried (the mirror alone changes) */
OSStatus LBAudioDetectiveResamplerBankResetChannels(LBAudioDetectiveResamplerBankRef inBank, const UInt32* inChannels, UInt32 inNumberOfChannels);
/* Debug / tests: the host plan of one call, needs no device.  Per channel, from inInputTotals samples received, inOutputTotals =
 * emitted(inInputTotals) samples emitted and inSampleCounts new ones: outNew = the samples the call emits -- emitted(total) -
 * emitted, or with inFinish != 0 n_out(total) - emitted --, outCarried = the samples the channel carries afterwards (0 with
 * inFinish); *outTapLow / *outTapHigh (may be NULL) = m_lo / m_hi.  ArgumentInvalid for a pair New refuses and for an output total
 * that is not the input total's. */
OSStatus LBAudioDetectiveDebugResamplerBankPlan(Float64 inInputSampleRate, Float64 inOutputSampleRate, UInt32 inResamplerMode,
                                                UInt32 inNumberOfChannels, const UInt64* inInputTotals, const UInt64* inOutputTotals,
                                                const UInt32* inSampleCounts, UInt32 inFinish, UInt32* outNew, UInt32* outCarried,
                                                SInt32* outTapLow, SInt32* outTapHigh);

/* Stage 2 alone: inFrames = device pointer to inNumberOfFrames x 128 x bands float32 frame rows (what
 * LBAudioDetectiveFrameSetRow collects upstream) -> packed sub-fingerprints; outFramesHaar (optional)
 * receives the decomposed frames.  Replaces LBAudioDetectiveSynthesizeFingerprint
 * (LBAudioDetective.m:315-331) for a batch of full frames. */
OSStatus LBAudioDetectiveFramesToSubfingerprintsDevice(LBAudioDetectiveRef inDetective, const Float32* inFrames,
                                                       UInt64 inNumberOfFrames, void* outPacked, Float32* outFramesHaar,
                                                       void* inStream);
/* Round 4: where more than half of the bands are structurally empty (a band whose bin range is empty is +0.0 in every
 * window: 17 of the 32 bands at 44.1 kHz / 1024-sample windows) and only one of bands 0..15 is live, the two kernels
 * exchange COMPACT frames -- 128 rows of ONLY the bands that can be non-zero: the live ones of bands 16..31 in ascending
 * order, then that one band (15 floats per row instead of 32 at 44.1 kHz / 1024; never more than 17, hence
 * LBAD_COMPACT_FRAME_FLOATS as an upper bound for buffers) -- and stage 2 runs a sparse form with the same results.
 * GetCompactLayout: noErr and the live left band (32: none) / the number of columns of the row transform that can be
 * non-zero, or ArgumentInvalid when the configuration has no such layout.  GetCompactBands: which bands a row holds, in
 * the order they are stored (outBands may be NULL; *outCount <= 17): a frame is 128 x *outCount floats.
 * CompactFramesToSubfingerprintsDevice: the sparse stage 2 alone on such frames (tests, fuzzers). */
#define LBAD_COMPACT_FRAME_FLOATS 2176
OSStatus LBAudioDetectiveGetCompactLayout(LBAudioDetectiveRef inDetective, UInt32* outLeftBand, UInt32* outLiveColumns);
OSStatus LBAudioDetectiveGetCompactBands(LBAudioDetectiveRef inDetective, UInt32* outBands, UInt32* outCount);
OSStatus LBAudioDetectiveCompactFramesToSubfingerprintsDevice(LBAudioDetectiveRef inDetective, const Float32* inFrames,
                                                              UInt64 inNumberOfFrames, void* outPacked,
                                                              Float32* outFramesHaar, void* inStream);

/* Boolean <-> packed conversion on the host (no arithmetic). */
void LBAudioDetectivePackSubfingerprint(const Boolean* inBooleans, UInt32 inLength, UInt32* outWords);
void LBAudioDetectiveUnpackSubfingerprint(const UInt32* inWords, UInt32 inLength, Boolean* outBooleans);

/* ---- device-resident reference corpus -------------------------------------------------- */
typedef struct LBAudioDetectiveCorpus* LBAudioDetectiveCorpusRef;

/* Every entry has inSubfingerprintsPerEntry sub-fingerprints of inSubfingerprintLength
 * Booleans; inCapacity entries of HBM are reserved up front. */
LBAudioDetectiveCorpusRef LBAudioDetectiveCorpusNew(UInt32 inSubfingerprintLength, UInt32 inSubfingerprintsPerEntry,
                                                    UInt64 inCapacity);
/* Ragged corpus: every entry has its own number (>= 1) of sub-fingerprints -- what the upstream best-match
 * loop actually compares (LBAudioDetectiveTests.m:57-91: one original against ten sequences, all of different
 * lengths; LBAudioDetectiveFingerprint.m:123-146 swaps the two sides and slides the shorter along the longer).
 * inSubfingerprintLength <= 200.  HBM for inSubfingerprintCapacity sub-fingerprints (32 bytes each) and
 * inEntryCapacity entries is reserved up front.  Every query entry point below accepts such a corpus and a query
 * of ANY number of sub-fingerprints; the scan is one launch (k_sliding.hip, k_sliding_short.hip). */
LBAudioDetectiveCorpusRef LBAudioDetectiveCorpusNewRagged(UInt32 inSubfingerprintLength, UInt64 inEntryCapacity,
                                                          UInt64 inSubfingerprintCapacity);
/* Append inNumberOfEntries entries to a ragged corpus: inPacked = device pointer to the entries' sub-fingerprints
 * back to back in the packed layout (sum(inCounts) x LBAD_PACKED_BYTES), inCounts = HOST array of the entries'
 * sub-fingerprint counts (each >= 1).  Asynchronous on inStream once the counts are read. */
OSStatus LBAudioDetectiveCorpusAppendRaggedPackedDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPacked,
                                                        const UInt32* inCounts, UInt64 inNumberOfEntries, void* inStream);
/* sub-fingerprints stored, over all entries */
UInt64 LBAudioDetectiveCorpusGetSubfingerprintTotal(LBAudioDetectiveCorpusRef inCorpus);
void LBAudioDetectiveCorpusDispose(LBAudioDetectiveCorpusRef inCorpus);
UInt64 LBAudioDetectiveCorpusGetCount(LBAudioDetectiveCorpusRef inCorpus);
/* bytes of HBM one entry occupies in the scan layout (ragged corpus: bytes per sub-fingerprint) */
UInt32 LBAudioDetectiveCorpusGetEntryStrideBytes(LBAudioDetectiveCorpusRef inCorpus);
/* Append entries from device memory in the packed batch layout
 * (inNumberOfEntries x perEntry x LBAD_PACKED_BYTES). */
OSStatus LBAudioDetectiveCorpusAppendPackedDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPacked,
                                                  UInt64 inNumberOfEntries, void* inStream);
/* Append one host fingerprint (exactly perEntry sub-fingerprints; any number >= 1 for a ragged corpus). */
OSStatus LBAudioDetectiveCorpusAppendFingerprint(LBAudioDetectiveCorpusRef inCorpus,
                                                 LBAudioDetectiveFingerprintRef inFingerprint);
/* Best-match loop of LBAudioDetectiveTests.m:57-91 over the corpus: the query is the fixed
 * first argument of LBAudioDetectiveFingerprintCompareToFingerprint, every entry the
 * second; strict '<' from 0.0 so the lowest index wins ties and *outIndex = -1 when
 * nothing scores above 0.  inRange == 0 means the sub-fingerprint length
 * (LBAudioDetective.m:443-445). */
OSStatus LBAudioDetectiveCorpusQuery(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                     UInt32 inRange, SInt64* outIndex, Float32* outScore);
/* Sharded form: scans this GPU's entries (global index = inIndexBase + local) and writes
 * ONE 64-bit key = (float bits of the best score << 32) | (0xFFFFFFFF - global index) to
 * the device pointer outKey (0 if the shard is empty).  max() over ranks of the keys
 * (e.g. an RCCL all-reduce with ncclMax on int64) is the global best match; decode with
 * LBAudioDetectiveCorpusDecodeKey.  Asynchronous on inStream. */
OSStatus LBAudioDetectiveCorpusQueryKeyDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                              UInt32 inRange, UInt64 inIndexBase, void* outKey, void* inStream);
void LBAudioDetectiveCorpusDecodeKey(UInt64 inKey, SInt64* outIndex, Float32* outScore);
/* Sharded query with the exchange step inside the library (one process per GPU, every rank holds a contiguous
 * index range of the corpus and calls this with the same query): scan of this rank's entries, then ONE
 * ncclAllReduce(count = number of queries, ncclUint64, ncclMax) of the keys over RCCL / xGMI on inStream, then the
 * 8-byte read-back; every rank receives the global best match, the lowest global index winning ties
 * (LBAudioDetectiveTests.m:80-83 across shards).  inComm is an ncclComm_t passed as void* -- the caller's own, or
 * one made with LBAudioDetectiveCommInitRank.  RCCL is loaded on first use (librccl.so.1; a copy already in the
 * process is reused).  ArgumentInvalid when inIndexBase + the shard's entry count exceeds 2^32 (the key carries
 * a 32-bit global index).  The call is COLLECTIVE: a rank whose own scan cannot run (that error, a NULL corpus, a
 * failed launch) still takes part in the exchange with empty keys, so the other ranks return their result, and
 * reports its own status afterwards; only a NULL communicator or a count of zero returns without the exchange
 * (nothing is allocated by the call: the key block belongs to the corpus). */
OSStatus LBAudioDetectiveCorpusQuerySharded(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                            UInt32 inRange, UInt64 inIndexBase, void* inComm, void* inStream,
                                            SInt64* outIndex, Float32* outScore);
OSStatus LBAudioDetectiveCorpusQueryBatchSharded(LBAudioDetectiveCorpusRef inCorpus,
                                                 const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                 UInt32 inRange, UInt64 inIndexBase, void* inComm, void* inStream,
                                                 SInt64* outIndices, Float32* outScores);
/* The same with the exchange step handed in: inAllReduce(inContext, keys, count, stream) must leave in `keys` (a
 * DEVICE array of `count` unsigned 64-bit words, in place) the element-wise MAXIMUM over all ranks, ordered on `stream`
 * -- what ncclAllReduce(keys, keys, count, ncclUint64, ncclMax, comm, stream) does; return noErr or an error status.
 * LBAudioDetectiveCorpusQueryBatchSharded is this function with RCCL's all-reduce.  For hosts that bring their own
 * collective (MPI, a different RCCL build) and for tests that run several "ranks" inside one process.  Batches of more
 * than LBAD_SHARD_KEYS queries run as several exchanges, cut the same way on every rank.  After the exchange has been
 * enqueued the call waits for the stream at most LBAudioDetectiveSetExchangeTimeout milliseconds (default 60 000,
 * 0 = for ever) and returns kLBAudioDetectiveCollectiveError when a peer never joined. */
#define LBAD_SHARD_KEYS 4096
typedef OSStatus (*LBAudioDetectiveAllReduceMaxFn)(void* inContext, UInt64* ioDeviceKeys, UInt32 inCount, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryBatchShardedWith(LBAudioDetectiveCorpusRef inCorpus,
                                                     const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                     UInt32 inRange, UInt64 inIndexBase,
                                                     LBAudioDetectiveAllReduceMaxFn inAllReduce, void* inContext,
                                                     void* inStream, SInt64* outIndices, Float32* outScores);
void LBAudioDetectiveSetExchangeTimeout(UInt32 inMilliseconds);

/* Ragged corpora, top-1 queries (no per-entry scores asked for): a match of 0.7 or better found anywhere in the scan is
 * published at once, and groups of sliding offsets whose sums can no longer reach it -- an upper bound: every remaining
 * sub-fingerprint ratio counted as 1 -- are not finished.  Exact: nothing that could win or tie is dropped, the result is
 * the full scan's (LBAudioDetectiveTests.m:57-91 keeps the best match only).  On by default; 0 switches it off (every
 * offset of every entry is evaluated, as when scores are requested). */
OSStatus LBAudioDetectiveCorpusSetBoundPruning(LBAudioDetectiveCorpusRef inCorpus, UInt32 inEnabled);
/* The score from which a match is published and bounds the rest of the scan (0 < score <= 1; default 0.7: unrelated
 * fingerprints score 0.5 +- 0.03, LBAudioDetective essay p.43).  The bound and its margin: a group of offsets is given up
 * when its largest sum so far + one point per remaining step < published score * query length * 0.999; with float32 sums of
 * at most 8192 terms the rounding of the sums stays three orders of magnitude inside that margin (k_sliding.hip:
 * kPruneMargin), longer queries are scanned without pruning. */
OSStatus LBAudioDetectiveCorpusSetBoundPruningThreshold(LBAudioDetectiveCorpusRef inCorpus, Float32 inScore);
Float32 LBAudioDetectiveCorpusGetBoundPruningThreshold(LBAudioDetectiveCorpusRef inCorpus);
/* the corpus' own key block of a sharded query (LBAD_SHARD_KEYS words on the device, and its pinned host twin) */
unsigned long long* LBAudioDetectiveCorpusShardKeysDevice(LBAudioDetectiveCorpusRef inCorpus);
unsigned long long* LBAudioDetectiveCorpusShardKeysHost(LBAudioDetectiveCorpusRef inCorpus);
/* Communicator helpers for hosts without an RCCL binding of their own: rank 0 obtains a 128-byte id
 * (LBAD_COMM_UNIQUE_ID_BYTES) and hands it to the other ranks by whatever means the host has (a file, a socket,
 * MPI, torch.distributed ...); then every rank calls InitRank with the current HIP device set.  Thin wrappers
 * of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy. */
#define LBAD_COMM_UNIQUE_ID_BYTES 128
OSStatus LBAudioDetectiveCommGetUniqueId(void* outUniqueId);
OSStatus LBAudioDetectiveCommInitRank(void** outComm, SInt32 inNumberOfRanks, const void* inUniqueId, SInt32 inRank);
OSStatus LBAudioDetectiveCommDestroy(void* inComm);
/* What the communicator itself says (ncclCommCount / ncclCommUserRank): the number of ranks that joined it and this
 * rank's number in it.  Round 6: a multi-rank run can check that the library's communicator -- not only the host's own
 * process group -- spans every rank (bench.py --gpus N refuses a line whose count differs from N and names the rank). */
OSStatus LBAudioDetectiveCommGetInfo(void* inComm, SInt32* outNumberOfRanks, SInt32* outRank);
/* Several queries against one pass over the corpus -- the shape of the reference's own test, Q originals against N
 * candidates (LBAudioDetectiveTests.m:57-91).  Uniform corpus: up to 8 queries share each read of an entry.  Ragged
 * corpus (round 5): queries of ONE length share their passes over the records, four per launch (eight in the scan of short
 * queries -- round 6: queries of up to 12 sub-fingerprints, eight per launch in a kernel of their own: eight queries of 5
 * cost 2.2 x one); a batch of mixed lengths runs one group per length.  Results are those of inCount separate
 * LBAudioDetectiveCorpusQuery calls, bit for bit.  The KeysDevice form writes inCount keys to the device pointer
 * outKeys for a sharded max-reduction. */
OSStatus LBAudioDetectiveCorpusQueryBatch(LBAudioDetectiveCorpusRef inCorpus, const LBAudioDetectiveFingerprintRef* inQueries,
                                          UInt32 inCount, UInt32 inRange, SInt64* outIndices, Float32* outScores);
OSStatus LBAudioDetectiveCorpusQueryBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus,
                                                    const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                    UInt32 inRange, UInt64 inIndexBase, void* outKeys, void* inStream);
/* Per-entry scores (debug / parity): device pointer to count float32. */
OSStatus LBAudioDetectiveCorpusScoresDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                            UInt32 inRange, Float32* outScores, void* inStream);
/* Top-K queries: the inK best matches per query, selected on the device.  Entry e scores exactly what
 * LBAudioDetectiveCorpusScoresDevice returns for it; the list holds the entries with score > 0, score descending, equal
 * scores lowest index first, cut at inK (K = 1 is LBAudioDetectiveCorpusQuery's answer, bit for bit).  *outCount =
 * min(inK, entries with score > 0); unused slots get index -1 and score 0.  1 <= inK <= LBAD_TOPK_MAX, inRange == 0 means
 * the sub-fingerprint length.  The batch forms write inCount x inK results (query q's list at q * inK) and inCount counts;
 * a batch equals inCount single calls, bit for bit.  The KeysDevice form writes inCount x inK 64-bit keys (as
 * LBAudioDetectiveCorpusQueryKeyDevice, global index = inIndexBase + local; each row descending, 0-padded) to the device
 * pointer outKeys, asynchronously on inStream; the keys of several shards merge by taking the K largest.  The corpus owns
 * the scratch (scores, histograms, candidates), grown on demand; a call waits for the previous top-K call's device work
 * before it reuses it. */
#define LBAD_TOPK_MAX 1024
OSStatus LBAudioDetectiveCorpusQueryTopK(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                         UInt32 inRange, UInt32 inK, SInt64* outIndices, Float32* outScores, UInt32* outCount);
OSStatus LBAudioDetectiveCorpusQueryBatchTopK(LBAudioDetectiveCorpusRef inCorpus, const LBAudioDetectiveFingerprintRef* inQueries,
                                              UInt32 inCount, UInt32 inRange, UInt32 inK,
                                              SInt64* outIndices, Float32* outScores, UInt32* outCounts);
OSStatus LBAudioDetectiveCorpusQueryBatchTopKKeysDevice(LBAudioDetectiveCorpusRef inCorpus,
                                                        const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                        UInt32 inRange, UInt32 inK, UInt64 inIndexBase,
                                                        void* outKeys, void* inStream);
/* The selection on its own: inRows rows of inCount float32 scores (device, row r at inScores + r * inCount) to inRows x inK
 * keys at the device pointer outKeys (index = inIndexBase + position in the row; inIndexBase + inCount <= 2^32).  Scores
 * that are <= 0 or NaN are never selected.  Allocates its own scratch and returns once the keys are written. */
OSStatus LBAudioDetectiveTopKKeysFromScoresDevice(const Float32* inScores, UInt64 inCount, UInt32 inRows, UInt32 inK,
                                                  UInt64 inIndexBase, void* outKeys, void* inStream);
/* Threshold queries: EVERY entry whose score reaches inThreshold, selected on the device -- "which entries match this query at
 * all" (unrelated fingerprints score 0.5 +- 0.03, a real match far above: 0.7 is the level bound pruning starts from as well).
 * Entry e scores exactly what LBAudioDetectiveCorpusScoresDevice returns for it and matches when score >= inThreshold as
 * Float32 values (a NaN never matches).  A row has inCapacity slots: the first min(count, inCapacity) matches in ASCENDING
 * entry index, then index -1, score 0 (and lag 0).  The count is always the TRUE number of matches: count > inCapacity tells
 * that the list was cut, which is no error.  inThreshold is finite and > 0 (above 1 is legal and matches nothing),
 * inCapacity >= 1, inCount x inCapacity <= 2^31, inRange == 0 means the sub-fingerprint length, queries of the corpus'
 * sub-fingerprint length, inIndexBase + entries <= 2^32; NULL handles and pointers are kLBAudioDetectiveArgumentInvalid, and
 * without a device every call returns kLBAudioDetectiveDeviceUnavailable.  An empty corpus gives counts 0, zero keys and zero
 * lags.  Bound pruning never applies (these are scores scans, as for top-K).  The batch forms write inCount x inCapacity
 * results (query q's list at q * inCapacity) and inCount counts; a batch equals inCount single calls, bit for bit.  The
 * Aligned form adds every match's lag (see below), equal to LBAudioDetectiveCorpusAlignKeysDevice's on the same keys.
 * The KeysDevice form writes inCount x inCapacity 64-bit keys (as the top-K calls', global index = inIndexBase + local; each
 * row in ascending index, 0-padded -- sort a row descending for best-first) to the device pointer outKeys and inCount UInt64
 * counts to the device pointer outCounts, asynchronously on inStream, which is never awaited.  Shards that hold contiguous
 * index ranges merge by concatenating their rows in rank order and adding their counts.  The Packed form takes its queries
 * as LBAudioDetectiveCorpusQueryPackedTopKKeysDevice does (nothing is copied to the host) and writes, unless outLags is NULL,
 * inCount x inCapacity SInt32 lags to the device pointer outLags; its keys and counts equal the KeysDevice form's.  The
 * scratch is the top-K calls' (scores, staged queries, its event) plus the selection's tile counts; a call waits for the
 * previous top-K or threshold call's device work before it reuses it. */
OSStatus LBAudioDetectiveCorpusQueryThreshold(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                              UInt32 inRange, Float32 inThreshold, UInt64 inCapacity, SInt64* outIndices,
                                              Float32* outScores, UInt64* outCount);
OSStatus LBAudioDetectiveCorpusQueryBatchThreshold(LBAudioDetectiveCorpusRef inCorpus,
                                                   const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount, UInt32 inRange,
                                                   Float32 inThreshold, UInt64 inCapacity, SInt64* outIndices, Float32* outScores,
                                                   UInt64* outCounts);
OSStatus LBAudioDetectiveCorpusQueryBatchThresholdAligned(LBAudioDetectiveCorpusRef inCorpus,
                                                          const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                          UInt32 inRange, Float32 inThreshold, UInt64 inCapacity, SInt64* outIndices,
                                                          Float32* outScores, SInt32* outLags, UInt64* outCounts);
OSStatus LBAudioDetectiveCorpusQueryBatchThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus,
                                                             const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                             UInt32 inRange, Float32 inThreshold, UInt64 inCapacity,
                                                             UInt64 inIndexBase, void* outKeys, void* outCounts, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                              UInt32 inCount, UInt32 inSubfingerprintsPerQuery, UInt32 inRange,
                                                              Float32 inThreshold, UInt64 inCapacity, UInt64 inIndexBase,
                                                              void* outKeys, void* outCounts, void* outLags, void* inStream);
/* The selection on its own: inRows rows of inCount float32 scores (device, row r at inScores + r * inCount; any 4-byte
 * aligned address) to inRows x inCapacity keys at outKeys and inRows UInt64 counts at outCounts (device pointers; index =
 * inIndexBase + position in the row, inIndexBase + inCount <= 2^32, inRows x inCapacity <= 2^31).  Allocates its own scratch
 * and returns once the keys are written. */
OSStatus LBAudioDetectiveThresholdKeysFromScoresDevice(const Float32* inScores, UInt64 inCount, UInt32 inRows, Float32 inThreshold,
                                                       UInt64 inCapacity, UInt64 inIndexBase, void* outKeys, void* outCounts,
                                                       void* inStream);
/* Corpus join: every pair (entry of inQueries used as a query, entry of inCorpus) whose score reaches inThreshold, found on the
 * device -- "which entries of this corpus match each other" (inQueries == inCorpus is allowed) and "which of these new entries
 * are in the main corpus already".  A row is one of the entries inFirstQuery .. inFirstQuery + inQueryCount - 1 of inQueries.
 * Row i against entry j scores exactly what LBAudioDetectiveCorpusScoresDevice writes for entry j with row i's fingerprint as
 * the query; the query supplies the non-zero pairs, so score(i -> j) != score(j -> i) in general and the join reports ORDERED
 * pairs.  A pair matches when score >= inThreshold as Float32 values.  The result is CSR over the rows: outOffsets receives
 * inQueryCount + 1 UInt64, offsets[r] = matches of the rows before r, offsets[inQueryCount] = the TRUE total, never cut;
 * outKeys receives inCapacity keys (score bits << 32 | 0xFFFFFFFF - (inIndexBase + j)): the match at position p (rows ascending,
 * entry index ascending inside a row) in slot p where p < inCapacity, zero keys behind min(total, inCapacity).  A total above
 * inCapacity tells that the list was cut, which is no error; the row of slot p is the last r with offsets[r] <= p.  The result
 * does not depend on launch order, grid or chunking.  inSkipSameIndex != 0 leaves out the pair whose row index (in inQueries)
 * equals the entry's index (in inCorpus): the self-match of a self-join.  Both corpora are uniform and of ONE shape, sub-
 * fingerprints of 200 Booleans and 1 .. 8 of them per entry; a ragged corpus, another shape or two different shapes are
 * kLBAudioDetectiveArgumentInvalid.  inThreshold is finite and > 0 (above 1 is legal and matches nothing), inQueryCount >= 1,
 * inFirstQuery + inQueryCount <= entries of inQueries, 1 <= inCapacity <= 2^31, inIndexBase + entries of inCorpus <= 2^32,
 * inRange == 0 means the sub-fingerprint length; NULL handles and pointers are kLBAudioDetectiveArgumentInvalid, and without a
 * device arguments that pass these checks get kLBAudioDetectiveDeviceUnavailable.  An empty inCorpus gives zero offsets and
 * keys.  Bound pruning and LBAudioDetectiveCorpusSetKernelVariant do not apply.
 * The KeysDevice form writes to device pointers, asynchronously on inStream, which it never awaits; the rows go through in
 * chunks with nothing visiting the host in between, and the call waits ON THE DEVICE for the latest append of either corpus.
 * LBAudioDetectiveCorpusJoinThreshold returns the first min(total, inCapacity) pairs to host arrays of inCapacity elements --
 * (row index in inQueries, entry index, score) -- then -1 / -1 / 0, and the total.
 * The scratch belongs to inCorpus: 16 + rows x (584 + 8 x tiles) + ceil(rows / 64) x 4 x tiles bytes for a chunk of `rows` rows
 * (a multiple of 64, or all the call's rows), tiles = ceil(entries of inCorpus / 256).  It grows on demand up to the limit set
 * with LBAudioDetectiveCorpusSetJoinScratchLimit (0 = the default, 256 MiB), which thereby sets the rows per chunk; a limit
 * below one chunk of 64 rows is kLBAudioDetectiveArgumentInvalid at the call.  A call waits for the previous join's device work
 * before it reuses the scratch. */
OSStatus LBAudioDetectiveCorpusJoinThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                                       UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange, Float32 inThreshold,
                                                       UInt32 inSkipSameIndex, UInt64 inCapacity, UInt64 inIndexBase, void* outKeys,
                                                       void* outOffsets, void* inStream);
OSStatus LBAudioDetectiveCorpusJoinThreshold(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                             UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange, Float32 inThreshold,
                                             UInt32 inSkipSameIndex, UInt64 inCapacity, SInt64* outQueryIndices,
                                             SInt64* outEntryIndices, Float32* outScores, UInt64* outTotal);
OSStatus LBAudioDetectiveCorpusSetJoinScratchLimit(LBAudioDetectiveCorpusRef inCorpus, UInt64 inBytes);   /* 0 = default */
/* The join of RAGGED corpora (LBAudioDetectiveCorpusNewRagged): the contract above, word for word, except for what follows.
 * Both corpora are ragged and of one sub-fingerprint length (inQueries == inCorpus is allowed); a uniform corpus on either
 * side, two sub-fingerprint lengths, or a longest entry above LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS in either corpus are
 * kLBAudioDetectiveArgumentInvalid (the cap bounds a pair's offsets and a tile's task count to 32 bits and lets a row live in
 * LDS; 1024 sub-fingerprints are a 25-minute recording at the default settings).  Row i against entry j scores, bit for bit,
 * what LBAudioDetectiveCorpusScoresDevice(inCorpus, copy of row i's fingerprint, inRange) writes for entry j: the shorter of
 * the two slides along the longer, fingerprint1 is the entry when the row is shorter and the row otherwise (equal lengths
 * included), score = max(0, max over the offsets of fl(fl(sum of the steps' hits / possible) / steps)), and a pair matches when
 * score >= inThreshold as Float32 -- the compare is on the quotient.  outLags (device, inCapacity SInt32, may be NULL; the host
 * form's outLags likewise) receives in slot p the signed lag of the match in slot p, the value
 * LBAudioDetectiveCorpusAlignKeysDevice gives for that row and key: +offset when the entry is longer than the row, -offset
 * otherwise, of the LOWEST offset that reaches the score; 0 behind the matches.  Keys and offsets do not depend on outLags.
 * Two facts about the ordered pairs, checked on the CPU oracle (260 synthetic entries of 1 .. 300 sub-fingerprints): for
 * entries of DIFFERENT lengths score(i -> j) and score(j -> i) are the same bits and the lags are opposite -- both directions
 * slide the shorter along the longer with the longer as fingerprint1; for EQUAL lengths they differ in general (956 of 1 174
 * equal-length cells did).  The join reports ordered pairs all the same.
 * The host form returns (row, entry, score, lag), then -1 / -1 / 0 / 0, and the total.  Bound pruning and
 * LBAudioDetectiveCorpusSetKernelVariant do not apply.
 * The scratch is inCorpus' join scratch, under LBAudioDetectiveCorpusSetJoinScratchLimit: 16 + rows x (8 + 8 x tiles) +
 * ceil(rows / 64) x 4 x tiles bytes for a chunk of `rows` rows (a multiple of 64, or all the call's rows), tiles =
 * ceil(entries of inCorpus / 256); the records of the rows and of inCorpus do not enter it.  A limit below one chunk of 64
 * rows is kLBAudioDetectiveArgumentInvalid at the call. */
#define LBAD_JOIN_RAGGED_MAX_SUBFINGERPRINTS 1024
OSStatus LBAudioDetectiveCorpusJoinRaggedThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                                             UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange,
                                                             Float32 inThreshold, UInt32 inSkipSameIndex, UInt64 inCapacity,
                                                             UInt64 inIndexBase, void* outKeys, void* outLags, void* outOffsets,
                                                             void* inStream);
OSStatus LBAudioDetectiveCorpusJoinRaggedThreshold(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveCorpusRef inQueries,
                                                   UInt64 inFirstQuery, UInt64 inQueryCount, UInt32 inRange, Float32 inThreshold,
                                                   UInt32 inSkipSameIndex, UInt64 inCapacity, SInt64* outQueryIndices,
                                                   SInt64* outEntryIndices, Float32* outScores, SInt32* outLags, UInt64* outTotal);
/* Occurrences: every place ONE query -- a long recording -- matches a RAGGED corpus, found on the device.  Every other corpus
 * call folds the sliding compare into one number per entry, max over the offsets; these calls return the cells themselves.  For
 * entry j the cells are the n1 - n2 + 1 values q_o that LBAudioDetectiveCorpusMatchProfile(inCorpus, inQuery, inRange, j) returns,
 * bit for bit: fingerprint1 is the entry when the query is shorter (lag +o), the query otherwise (equal lengths included, lag
 * -o), q_o = fl(fl(sum of the steps' hits / possible, in step order from +0) / n2), possible from fingerprint1's pairs inside the
 * range.  A cell matches when q_o >= inThreshold as Float32; with inPeaksOnly != 0 it must also be a local peak of its own
 * profile, (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)) as Float32 -- a plateau reports its first cell only, cells
 * outside the profile do not exist, and a neighbour below the threshold still takes part in the test.
 * outKeys receives inCapacity 64-bit keys, q_o bits << 32 | 0xFFFFFFFF - (inIndexBase + j), the key format of every other call;
 * outLags (may be NULL) inCapacity SInt32 signed lags; outCount one UInt64, the TRUE number of matching cells, never cut -- a
 * count above inCapacity is no error.  The matches lie in ascending entry index and inside an entry in ascending offset o (with
 * the query as fingerprint1 that is descending lag); slot p < min(count, capacity) holds match p, every slot behind a zero key
 * and lag 0.  Keys and count do not depend on outLags, launch order, grid or chunking.  Shards that hold contiguous index ranges
 * merge by concatenating in rank order and adding counts.
 * The corpus is ragged (a uniform corpus is kLBAudioDetectiveArgumentInvalid: gather it into a ragged one) with no entry above
 * LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS; the query has the corpus' sub-fingerprint length and 1 .. 2^31 - 1 sub-
 * fingerprints; inThreshold is finite and > 0 (above 1 is legal and matches nothing), 1 <= inCapacity <= 2^31, inIndexBase +
 * entries <= 2^32, inRange == 0 means the sub-fingerprint length; NULL handles and pointers but outLags are
 * kLBAudioDetectiveArgumentInvalid.  What needs no handle is refused first, then kLBAudioDetectiveDeviceUnavailable, then what
 * needs the corpus.  An empty corpus gives count 0 and zero keys and lags.
 * The KeysDevice forms write to device pointers, asynchronously on inStream, which they never await, and wait ON THE DEVICE
 * for the corpus' latest append.  The Packed form takes the query as inSubfingerprints x LBAD_PACKED_BYTES bytes on the device
 * (4-byte aligned, bits at or above the sub-fingerprint length ignored; nothing of it visits the host); its keys, lags and count
 * equal the handle form's bit for bit.  LBAudioDetectiveCorpusQueryOccurrences returns (index, score, lag) of the first
 * min(count, inCapacity) matches to host arrays of inCapacity elements, then -1 / 0 / 0, and the count.
 * The scratch is the corpus' join scratch, under LBAudioDetectiveCorpusSetJoinScratchLimit: the entries go through in chunks of
 * a multiple of 64 with nothing visiting the host in between, 24 + entries x (16 + 8 x tiles) + ceil(entries / 64) x
 * ceil(tiles / 4) x 4 bytes for a chunk, tiles = ceil(most offsets of any pair / 126); a limit below one chunk of 64 entries is
 * kLBAudioDetectiveArgumentInvalid at the call. */
#define LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS 1024
OSStatus LBAudioDetectiveCorpusQueryOccurrencesKeysDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                                          UInt32 inRange, Float32 inThreshold, UInt32 inPeaksOnly, UInt64 inCapacity,
                                                          UInt64 inIndexBase, void* outKeys, void* outLags, void* outCount,
                                                          void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQuery,
                                                                UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                UInt32 inPeaksOnly, UInt64 inCapacity, UInt64 inIndexBase,
                                                                void* outKeys, void* outLags, void* outCount, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryOccurrences(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                                UInt32 inRange, Float32 inThreshold, UInt32 inPeaksOnly, UInt64 inCapacity,
                                                SInt64* outIndices, Float32* outScores, SInt32* outLags, UInt64* outCount);
/* Recording scores: how well EVERY entry of a RAGGED corpus matches ONE query of any length -- a long recording above all --
 * and where, with the occurrences pass' pair loop: a pair whose entry is the shorter side takes as many steps as the entry has
 * sub-fingerprints, not as many as the query (the ragged scan behind LBAudioDetectiveCorpusScoresDevice was built for queries of
 * about a hundred sub-fingerprints).  The cells of the occurrences calls above are folded per entry on the device.
 * SCORES: outScores[j] is, bit for bit, what LBAudioDetectiveCorpusScoresDevice writes for entry j with the same query and
 * range: the largest cell q_o of the pair's profile (cells are >= +0, which is the scan's max(0, .)).
 * LAGS: outLags[j] (may be NULL; the scores do not depend on it) is what LBAudioDetectiveCorpusAlignKeysDevice gives for that
 * entry: the LOWEST offset o whose cell equals the score, +o when the entry is longer than the query and -o otherwise (equal
 * lengths included).  A score of 0 means every cell is 0: the lag is 0.
 * LBAudioDetectiveCorpusRecordingScoresDevice / ...RecordingPackedScoresDevice write one Float32 and one SInt32 per entry to
 * device pointers.  The key forms run the same pass into the corpus' scores scratch, then the selections of the top-K and
 * threshold queries as they are, then gather the selected entries' lags:
 * ...QueryPackedRecordingTopKKeysDevice writes inK keys (and lags) that equal LBAudioDetectiveCorpusQueryPackedTopKKeysDevice's
 * with one query -- K = 1 is the top-1 query's answer --, ...QueryPackedRecordingThresholdKeysDevice inCapacity keys (and lags)
 * and one UInt64 count that equal LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice's with one query; a zero key has lag 0.
 * LBAudioDetectiveCorpusQueryRecordingTopK returns (index, score, lag) of the inK best entries to host arrays of inK elements
 * (outLags may be NULL), unused slots -1 / 0 / 0, and *outCount = min(inK, entries with score > 0).
 * The restrictions are the occurrences calls': the corpus is ragged (a uniform corpus is kLBAudioDetectiveArgumentInvalid) with
 * no entry above LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS; the query has the corpus' sub-fingerprint length and 1 .. 2^31 - 1
 * sub-fingerprints, short ones included; inRange == 0 means the sub-fingerprint length; 1 <= inK <= LBAD_TOPK_MAX; inThreshold
 * is finite and > 0, 1 <= inCapacity <= 2^31, inIndexBase + entries <= 2^32; NULL handles and pointers but outLags are
 * kLBAudioDetectiveArgumentInvalid.  What needs no handle is refused first, then kLBAudioDetectiveDeviceUnavailable, then what
 * needs the corpus.  An empty corpus is noErr: the scores forms write nothing, the key forms zero keys, lags and count.
 * The Device forms are asynchronous on inStream, which they never await, and wait ON THE DEVICE for the corpus' latest append.
 * The Packed forms take the query as inSubfingerprints x LBAD_PACKED_BYTES bytes on the device (4-byte aligned, bits at or above
 * the sub-fingerprint length ignored; nothing of it visits the host); packed, handle and host forms agree bit for bit.  Bound
 * pruning and LBAudioDetectiveCorpusSetKernelVariant do not apply.  Results do not depend on launch order, grid or chunking.
 * The scratch is the corpus' join scratch, under LBAudioDetectiveCorpusSetJoinScratchLimit: the entries go through in chunks of
 * a multiple of 64 with nothing visiting the host in between, entries x tiles x 8 bytes for a chunk, tiles = ceil(most offsets
 * of any pair / 126); a limit below one chunk of 64 entries is kLBAudioDetectiveArgumentInvalid at the call. */
OSStatus LBAudioDetectiveCorpusRecordingScoresDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                                     UInt32 inRange, Float32* outScores, SInt32* outLags, void* inStream);
OSStatus LBAudioDetectiveCorpusRecordingPackedScoresDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQuery,
                                                           UInt32 inSubfingerprints, UInt32 inRange, Float32* outScores,
                                                           SInt32* outLags, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryRecordingTopK(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                                  UInt32 inRange, UInt32 inK, SInt64* outIndices, Float32* outScores,
                                                  SInt32* outLags, UInt32* outCount);
OSStatus LBAudioDetectiveCorpusQueryPackedRecordingTopKKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQuery,
                                                                  UInt32 inSubfingerprints, UInt32 inRange, UInt32 inK,
                                                                  UInt64 inIndexBase, void* outKeys, void* outLags, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedRecordingThresholdKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQuery,
                                                                       UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                       UInt64 inCapacity, UInt64 inIndexBase, void* outKeys,
                                                                       void* outCount, void* outLags, void* inStream);
/* Recording timeline: what was playing at each moment of ONE query -- a long recording -- against a RAGGED corpus: the cells of
 * the occurrences calls above folded per OFFSET of the query over the entries, on the device.  The output is bounded by the
 * recording, one 64-bit key per sub-fingerprint offset, whatever the corpus size.
 * Entry j of n_j sub-fingerprints TAKES PART when n_j <= n_q, the query's sub-fingerprints (the query is fingerprint1, equal
 * lengths included); a longer entry has no position inside the recording and is skipped.  The cells of a participating entry are
 * the n_q - n_j + 1 values q_o(j) that LBAudioDetectiveCorpusMatchProfile(inCorpus, inQuery, inRange, j) returns, bit for bit; o
 * is the sub-fingerprint of the recording at which the entry starts.  A cell COUNTS when q_o(j) >= inThreshold as Float32.
 * KEYS: outKeys[o], for every o in [0, n_q), is the unsigned maximum over the counting cells of
 * q_o(j) bits << 32 | 0xFFFFFFFF - (inIndexBase + j), the key format of every other call (LBAudioDetectiveCorpusDecodeKey,
 * ...GatherKeysDevice and ...RemoveKeysDevice accept it): the best score, ties to the LOWEST entry index; 0 where no cell counts.
 * All n_q words are written.
 * LENGTHS: outLengths[o] (n_q UInt32, may be NULL; the keys do not depend on it) is n_j of the winning entry -- it spans
 * [o, o + n_j) of the recording --, 0 for a zero key.
 * Shards that hold contiguous index ranges merge by the element-wise unsigned maximum of their key arrays (the lengths follow
 * the winning shard's).
 * The restrictions are the occurrences calls': the corpus is ragged (a uniform corpus is kLBAudioDetectiveArgumentInvalid) with
 * no entry above LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS; the query has the corpus' sub-fingerprint length and 1 .. 2^31 - 1
 * sub-fingerprints; inThreshold is finite and > 0 (a zero cell never counts; above 1 is legal and matches nothing), inIndexBase +
 * entries <= 2^32, inRange == 0 means the sub-fingerprint length; NULL handles and pointers but outLengths are
 * kLBAudioDetectiveArgumentInvalid.  What needs no handle is refused first, then kLBAudioDetectiveDeviceUnavailable, then what
 * needs the corpus.  An empty corpus, and a corpus without a participating entry, are noErr with zero keys and lengths.
 * The Device forms are asynchronous on inStream, which they never await, and wait ON THE DEVICE for the corpus' latest append.
 * The Packed form takes the query as inSubfingerprints x LBAD_PACKED_BYTES bytes on the device (4-byte aligned, bits at or above
 * the sub-fingerprint length ignored; nothing of it visits the host); packed, handle and host forms agree bit for bit.
 * LBAudioDetectiveCorpusQueryRecordingTimeline returns (index, score, length) per offset to host arrays of n_q elements
 * (outLengths may be NULL), -1 / 0 / 0 where nothing counts, and *outCount = the offsets with a winner.  Results do not depend
 * on launch order, grid, chunking or outLengths; there is no early exit: every cell of every participating pair is computed.
 * The scratch is the corpus' join scratch, under LBAudioDetectiveCorpusSetJoinScratchLimit: the entries go through in chunks of
 * a multiple of 128 with nothing visiting the host in between, ceil(entries / 128) x tiles x 126 x 8 bytes for a chunk, tiles =
 * ceil((n_q - min(n_q, shortest entry) + 1) / 126); a limit below one chunk of 128 entries is kLBAudioDetectiveArgumentInvalid at
 * the call. */
OSStatus LBAudioDetectiveCorpusRecordingTimelineKeysDevice(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                                           UInt32 inRange, Float32 inThreshold, UInt64 inIndexBase, void* outKeys,
                                                           void* outLengths, void* inStream);
OSStatus LBAudioDetectiveCorpusRecordingPackedTimelineKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQuery,
                                                                 UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                 UInt64 inIndexBase, void* outKeys, void* outLengths,
                                                                 void* inStream);
OSStatus LBAudioDetectiveCorpusQueryRecordingTimeline(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                                      UInt32 inRange, Float32 inThreshold, SInt64* outIndices, Float32* outScores,
                                                      UInt32* outLengths, UInt64* outCount);
/* Batch recording timeline: the timeline above for MANY recordings of ONE length in one call -- what plays on every channel of a
 * broadcast monitor: hundreds to thousands of short windows against a small corpus, where one recording alone leaves the device
 * idle almost everywhere.  inPackedQueries is on the DEVICE, [inRecordings][inSubfingerprints][LBAD_PACKED_BYTES], 4-byte
 * aligned: exactly what LBAudioDetectiveStreamBankWindowDevice and LBAudioDetectiveFingerprintClipsDevice write.  outKeys (DEVICE,
 * [inRecordings][inSubfingerprints] UInt64) and outLengths (DEVICE, the same shape in UInt32, may be NULL; the keys do not depend
 * on it): row r of both is what LBAudioDetectiveCorpusRecordingPackedTimelineKeysDevice writes for recording r alone with the
 * same other arguments -- the key format, ties to the lowest entry index, zeros where nothing counts, every word written -- bit
 * for bit.  No record of recording r + 1 or r - 1 ever enters a cell of recording r.
 * The restrictions and the order of refusals are the single call's (a ragged corpus, no entry above
 * LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS, inThreshold finite and > 0, inIndexBase + entries <= 2^32; what needs no handle
 * first, then kLBAudioDetectiveDeviceUnavailable, then what needs the corpus); in addition inRecordings >= 1 and inRecordings x
 * inSubfingerprints <= 2^31 - 1.  An empty corpus, or one without a participating entry, is noErr with zero keys and lengths.
 * Asynchronous on inStream, which it never awaits; it waits ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * Results do not depend on launch order, grid, chunking, the kernel form or outLengths.
 * The scratch is the corpus' join scratch under LBAudioDetectiveCorpusSetJoinScratchLimit.  A call runs in PASSES over recordings
 * and, within a pass, in chunks over entries: where one recording's partials of the whole corpus (the single call's formula) fit
 * the limit, a pass takes min(inRecordings, limit / that) recordings in one chunk; otherwise one recording per pass, its entries
 * chunked as the single call chunks them.  A limit below one block of 128 entries for ONE recording is
 * kLBAudioDetectiveArgumentInvalid at the call.  Two kernel forms, chosen by the plan alone: form S (0), the single call's mapping
 * with the recording as one more coordinate; form W (1), a window per wave, when a recording has fewer than 4 tiles and four
 * windows of (126 + 2 + longest entry) records x 36 bytes plus the 20 604-byte table fit 160 KiB - 64 bytes of LDS.
 * LBAudioDetectiveDebugTimelineBatchPlan is that plan on the host -- the call takes its own from the same function --; it needs
 * neither device nor handle: from the shape of a call (inShortestEntry <= inLongestEntry <= the cap; inScratchLimit 0: the
 * default) the form, the tiles per recording, the recordings per pass, the entries per chunk, the scratch of a pass and the LDS
 * of a workgroup; kLBAudioDetectiveArgumentInvalid for a shape the call refuses, a limit that is too small or a NULL pointer.
 * LBAudioDetectiveDebugSetTimelineBatchForm (measurements and tests; process-wide, needs no device): non-zero makes every later
 * plan take form S where form W would be chosen, 0 restores the choice.  Results never depend on it. */
OSStatus LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                      UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                      Float32 inThreshold, UInt64 inIndexBase, void* outKeys,
                                                                      void* outLengths, void* inStream);
OSStatus LBAudioDetectiveDebugTimelineBatchPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry,
                                                UInt32 inLongestEntry, UInt64 inEntries, UInt64 inScratchLimit, UInt32* outForm,
                                                UInt64* outTiles, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                                                UInt64* outScratchBytes, UInt64* outLdsBytes);
OSStatus LBAudioDetectiveDebugSetTimelineBatchForm(UInt32 inForceShared);
/* Batch recording scores and batch recording top-K: the recording scores and the recording top-K above for MANY recordings of ONE
 * length in one call -- which entries the window of every channel of a broadcast monitor matches best, and where.
 * inPackedQueries is on the DEVICE, [inRecordings][inSubfingerprints][LBAD_PACKED_BYTES], 4-byte aligned: exactly what
 * LBAudioDetectiveStreamBankWindowDevice and LBAudioDetectiveFingerprintClipsDevice write.
 * LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice: outScores (DEVICE, [inRecordings][entries] Float32) and outLags (DEVICE,
 * the same shape in SInt32, may be NULL; the scores do not depend on it): row r of both is what
 * LBAudioDetectiveCorpusRecordingPackedScoresDevice writes for recording r alone, bit for bit; every word is written.
 * LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice: outKeys (DEVICE, [inRecordings][inK] UInt64) and outLags (DEVICE,
 * the same shape in SInt32, may be NULL): row r of both is what LBAudioDetectiveCorpusQueryPackedRecordingTopKKeysDevice writes for
 * recording r alone -- and therefore what LBAudioDetectiveCorpusQueryPackedTopKKeysDevice writes for query r of inRecordings, keys
 * and lags -- bit for bit: the same selection (score > 0, descending, the lowest index first, zero keys behind), run once per pass
 * with one row per recording.  Entries longer than the recordings take part, as in the single calls: the recording slides along
 * them.  No record of recording r + 1 or r - 1 ever enters a cell of recording r.
 * The restrictions and the order of refusals are the single calls' (a ragged corpus, no entry above
 * LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS, 1 <= inK <= LBAD_TOPK_MAX, inIndexBase + entries <= 2^32; what needs no handle first,
 * then kLBAudioDetectiveDeviceUnavailable, then what needs the corpus); in addition inRecordings >= 1, inRecordings x
 * inSubfingerprints <= 2^31 - 1, inRecordings x inK <= 2^31 and, in the scores form, inRecordings x entries <= 2^31 - 1.  An empty
 * corpus is noErr: the scores form writes nothing, the key form zero keys and lags.
 * Asynchronous on inStream, which it never awaits; it waits ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * Results do not depend on launch order, grid, chunking, the kernel form or outLags.
 * The scratch is the corpus' join scratch under LBAudioDetectiveCorpusSetJoinScratchLimit.  A call runs in PASSES over recordings
 * and, within a pass, in chunks over entries: where one recording's partials of the whole corpus (the single call's formula,
 * entries rounded up to 64 x tiles x 8 bytes, tiles as for the occurrences) fit the limit, a pass takes the smallest of
 * inRecordings, limit / that, (2^32 - 4097) / (entries x tiles), 65 535 and -- in the key form -- max(1, limit / (entries x 8)), the
 * rows of scores and lags the selection reads, in one chunk; otherwise one recording per pass, its entries chunked as the single
 * call chunks them.  A limit below one block of 64 entries for ONE recording is kLBAudioDetectiveArgumentInvalid at the call.  Two
 * kernel forms, chosen by the plan alone: form S (0), the single call's mapping with the recording as one more coordinate; form W
 * (1), a window per wave, when a recording has fewer than 4 tiles and four windows of (126 + 2 + longest entry) records x 36 bytes
 * plus the 20 604-byte table fit 160 KiB - 64 bytes of LDS.
 * LBAudioDetectiveDebugRecordingBatchPlan is that plan on the host -- the calls take their own from the same function --; it needs
 * neither device nor handle: from the shape of a call (inShortestEntry <= inLongestEntry <= the cap; inScratchLimit 0: the
 * default; inKeyForm non-zero: the top-K call's plan) the form, the tiles per recording, the recordings per pass, the entries per
 * chunk, the scratch of a pass and the LDS of a workgroup; kLBAudioDetectiveArgumentInvalid for a shape the call refuses, a limit
 * that is too small or a NULL pointer.
 * LBAudioDetectiveDebugSetRecordingBatchForm (measurements and tests; process-wide, needs no device; independent of the batch
 * timeline's switch): non-zero makes every later plan take form S where form W would be chosen, 0 restores the choice.  Results
 * never depend on it. */
OSStatus LBAudioDetectiveCorpusRecordingPackedScoresBatchDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                Float32* outScores, SInt32* outLags, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedRecordingTopKBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                       UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                       UInt32 inK, UInt64 inIndexBase, void* outKeys, void* outLags,
                                                                       void* inStream);
OSStatus LBAudioDetectiveDebugRecordingBatchPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry,
                                                 UInt32 inLongestEntry, UInt64 inEntries, UInt64 inScratchLimit, UInt32 inKeyForm,
                                                 UInt32* outForm, UInt64* outTiles, UInt32* outRecordingsPerPass,
                                                 UInt64* outEntriesPerChunk, UInt64* outScratchBytes, UInt64* outLdsBytes);
OSStatus LBAudioDetectiveDebugSetRecordingBatchForm(UInt32 inForceShared);
/* Batch occurrences and batch recording threshold: the occurrences and the recording threshold above for MANY recordings of ONE
 * length in one call -- every place the window of every channel of a broadcast monitor matches, at or above a score: an event per
 * (channel, entry, position), or per (channel, entry), with no K to guess.
 * inPackedQueries is on the DEVICE, [inRecordings][inSubfingerprints][LBAD_PACKED_BYTES], 4-byte aligned: exactly what
 * LBAudioDetectiveStreamBankWindowDevice and LBAudioDetectiveFingerprintClipsDevice write.  outKeys (DEVICE, [inRecordings]
 * [inCapacity] UInt64), outLags (DEVICE, the same shape in SInt32, may be NULL; keys and counts do not depend on it) and outCounts
 * (DEVICE, [inRecordings] UInt64); every word of all three is written.
 * LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice: row r of keys and lags, and outCounts[r], are what
 * LBAudioDetectiveCorpusQueryPackedOccurrencesKeysDevice writes for recording r alone with the same other arguments, bit for bit:
 * the key format, the (entry, offset) order, the peak rule with its plateaus (inPeaksOnly), zero keys and lags behind
 * min(count, inCapacity), the TRUE count never cut.  Entries longer than the recordings take part, as in the single call: the
 * recording slides along them.  No record of recording r + 1 or r - 1 ever enters a cell of recording r, and a row that overflows
 * writes nothing into its neighbours' slots.
 * LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice: row r is what
 * LBAudioDetectiveCorpusQueryPackedRecordingThresholdKeysDevice writes for recording r alone -- ascending index, the true count,
 * the lags aligned with the keys, lag 0 for a zero key -- and therefore what LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice
 * writes for query r of inRecordings.
 * The restrictions and the order of refusals are the single calls' (a ragged corpus, no entry above
 * LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS, inThreshold finite and > 0, 1 <= inCapacity <= 2^31, inIndexBase + entries <= 2^32;
 * what needs no handle first, then kLBAudioDetectiveDeviceUnavailable, then what needs the corpus); in addition inRecordings >= 1,
 * inRecordings x inSubfingerprints <= 2^31 - 1 and inRecordings x inCapacity <= 2^31.  An empty corpus is noErr with zero keys,
 * lags and counts.
 * Asynchronous on inStream, which they never await; they wait ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * Results do not depend on launch order, grid, chunking, the kernel form or outLags.  Shards that hold contiguous index ranges
 * merge per recording: the rows concatenated in rank order, the counts added.
 * The scratch is the corpus' join scratch under LBAudioDetectiveCorpusSetJoinScratchLimit.  A call runs in PASSES over recordings.
 * The occurrences: where one recording's scratch for the whole corpus (the single call's formula: 24 + entries rounded up to 64 x
 * (16 + 8 x tiles) + entry blocks of 64 x groups of 4 tiles x 4 bytes) fits the limit, a pass takes the smallest of inRecordings,
 * limit / that scratch, (2^32 - 4097) / (entries x tiles) and 65 535 recordings in one chunk, with that scratch per recording;
 * otherwise one recording per pass, its entries chunked as the single call chunks them, the running total carried from chunk to
 * chunk.  With one recording the tiles, the chunk and the scratch are the single call's.  A limit below one block of 64 entries
 * for ONE recording is kLBAudioDetectiveArgumentInvalid at the call.  Two kernel forms, chosen by the plan alone: form S (0), the
 * single call's unit with the recording as one more coordinate; form W (1), a window per wave, when a recording has fewer than 4
 * tiles and four windows of (126 + 2 + longest entry) records x 36 bytes plus the 20 604-byte table fit 160 KiB - 64 bytes of LDS.
 * The recording threshold: the passes, the chunks and the scratch of the batch recording top-K above (its key form), then one
 * compaction per pass over a row per recording -- the number of launches of a pass does not grow with the recordings.
 * LBAudioDetectiveDebugOccurrencesBatchPlan is the occurrences' plan on the host -- the call takes its own from the same function
 * --; it needs neither device nor handle: from the shape of a call (inShortestEntry <= inLongestEntry <= the cap; inScratchLimit
 * 0: the default) the form, the tiles per recording, the recordings per pass, the entries per chunk, the scratch of a pass and the
 * LDS of a workgroup; kLBAudioDetectiveArgumentInvalid for a shape the call refuses, a limit that is too small or a NULL pointer.
 * LBAudioDetectiveDebugSetOccurrencesBatchForm (measurements and tests; process-wide, needs no device; independent of the other
 * batch calls' switches): non-zero makes every later plan of these two calls take form S where form W would be chosen, 0 restores
 * the choice.  Results never depend on it. */
OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                     UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inRange,
                                                                     Float32 inThreshold, UInt32 inPeaksOnly, UInt64 inCapacity,
                                                                     UInt64 inIndexBase, void* outKeys, void* outLags, void* outCounts,
                                                                     void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedRecordingThresholdBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus,
                                                                            const void* inPackedQueries, UInt32 inRecordings,
                                                                            UInt32 inSubfingerprints, UInt32 inRange, Float32 inThreshold,
                                                                            UInt64 inCapacity, UInt64 inIndexBase, void* outKeys,
                                                                            void* outCounts, void* outLags, void* inStream);
OSStatus LBAudioDetectiveDebugOccurrencesBatchPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry,
                                                   UInt32 inLongestEntry, UInt64 inEntries, UInt64 inScratchLimit, UInt32* outForm,
                                                   UInt64* outTiles, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                                                   UInt64* outScratchBytes, UInt64* outLdsBytes);
OSStatus LBAudioDetectiveDebugSetOccurrencesBatchForm(UInt32 inForceShared);
/* Live occurrences: of the batch occurrences above only the cells a push has COMPLETED, for a monitor that asks after every push
 * and wants each match once.  inPackedQueries, outKeys, outLags (may be NULL) and outCounts are exactly
 * LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice's, on the DEVICE: inRecordings recordings of inSubfingerprints packed
 * sub-fingerprints each, keys and lags [inRecordings][inCapacity], counts UInt64 [inRecordings]; every word is written.
 * inNewCounts is on the DEVICE too: UInt32 [inRecordings], 4-byte aligned, read on the stream -- how many of recording r's
 * sub-fingerprints are new since the caller last asked (what a stream bank's push returned).  Recording r uses d_r =
 * min(inNewCounts[r], inMaxNew, inSubfingerprints).  inMaxNew is the HOST's bound, 1 <= inMaxNew <= LBAD_OCCURRENCES_TAIL_MAX_NEW:
 * it sizes the launch, and a device value above it counts as inMaxNew -- a caller whose push may complete more keeps the bound
 * at least that large, or the cells behind the newest inMaxNew are never reported.
 * Entry j of n_j sub-fingerprints takes part when n_j <= inSubfingerprints (the recording is fingerprint1, equal lengths included:
 * the timeline's rule); a longer entry has no complete position inside the recording and is skipped.  The cells of (r, j) are the
 * offsets o with max(0, inSubfingerprints - n_j - d_r + 1) <= o <= inSubfingerprints - n_j: the positions at which the entry ENDS
 * inside the newest d_r sub-fingerprints; d_r == 0: none.  A cell's value is q_o of LBAudioDetectiveCorpusMatchProfile, bit for
 * bit; it matches when q_o >= inThreshold as Float32.  There is NO peak rule: a newest cell's right neighbour does not exist yet.
 * Row r is, bit for bit, row r of the batch occurrences call with inPeaksOnly = 0 and the same other arguments with only those
 * cells kept: keys q_o bits << 32 | 0xFFFFFFFF - (inIndexBase + j), lags -o, in (entry ascending, offset ascending) order, zero
 * keys and lags 0 behind min(count, inCapacity); outCounts[r] is the TRUE number of matching cells, never cut; a row that
 * overflows writes nothing into its neighbours, and no sub-fingerprint of recording r +- 1 enters a cell of r.  Shards merge per
 * recording by concatenation, as the batch occurrences do.
 * EXACTLY ONCE: a cell's value depends only on the entry and the n_j sub-fingerprints under it.  So for a channel fed in pushes of
 * d_1, d_2, ... whose window at call k is at least (longest entry + d_k - 1) long, the cells of all calls moved to absolute
 * positions (total - inSubfingerprints + o) are the cells of ONE occurrences call (peaks off) over the whole recording, for the
 * entries not longer than the windows: each appears in exactly one call, with equal key bits.
 * Refusals in the batch call's order: what needs no handle first (a NULL pointer other than outLags, inNewCounts not 4-byte aligned,
 * inMaxNew 0 or above the cap, and the batch call's own argument checks), then kLBAudioDetectiveDeviceUnavailable, then what needs
 * the corpus (ragged, no entry above LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS, the sub-fingerprint length, a scratch limit --
 * LBAudioDetectiveCorpusSetJoinScratchLimit -- below one block of 64 entries for ONE recording).  An empty corpus, or one with no
 * entry that takes part, is noErr with zero keys, lags and counts.
 * Asynchronous on inStream, which it never awaits; it waits ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * Results do not depend on launch order, grid, chunking, passes or outLags.  The work is proportional to d x the entries' summed
 * lengths, not to the window.
 * LBAudioDetectiveDebugOccurrencesTailPlan is the call's plan on the host -- the call takes its own from the same function --; it
 * needs neither device nor handle: from the shape of a call (inShortestEntry <= inLongestEntry <= the cap; inScratchLimit 0: the
 * default) the lanes per recording D (the next power of two >= inMaxNew), the recordings per workgroup (256 / D, fewer where that
 * many windows do not fit the LDS), the records of a recording's LDS window (min(inSubfingerprints, min(longest entry,
 * inSubfingerprints) + D - 1)), the LDS of a workgroup (recordings x window x 36 bytes + the 20 604-byte table, at most 160 KiB - 64),
 * the recordings per pass, the entries per chunk and the scratch of a pass (the occurrences' formula with one tile, per recording;
 * at most 65 535 recordings a pass; one recording per pass in entry chunks when a whole corpus' scratch does not fit);
 * kLBAudioDetectiveArgumentInvalid for a shape the call refuses, a limit that is too small or a NULL pointer. */
#define LBAD_OCCURRENCES_TAIL_MAX_NEW 64
OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                         UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                         const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                         Float32 inThreshold, UInt64 inCapacity, UInt64 inIndexBase,
                                                                         void* outKeys, void* outLags, void* outCounts, void* inStream);
OSStatus LBAudioDetectiveDebugOccurrencesTailPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry,
                                                  UInt32 inLongestEntry, UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit,
                                                  UInt32* outLanes, UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords,
                                                  UInt64* outLdsBytes, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                                                  UInt64* outScratchBytes);
/* Live peaks: the live occurrences above under the occurrences' PEAK RULE -- one event per airing, each once in a channel's life.
 * The right neighbour of a cell exists one sub-fingerprint later, so this call judges every cell ONE SUB-FINGERPRINT LATE.  Every
 * argument except inFinal is LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice's: queries, new counts (UInt32
 * [inRecordings], 4-byte aligned, read on the stream) and outputs on the DEVICE, keys and lags [inRecordings][inCapacity], counts
 * UInt64 [inRecordings], every word written.  With n = inSubfingerprints, d_r = min(inNewCounts[r], inMaxNew, n), 1 <= inMaxNew <=
 * LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW (62: a recording takes inMaxNew + 2 lanes of one wave of 64).  Entry j of n_j sub-fingerprints
 * takes part when 1 <= n_j <= n; last = n - n_j.  The JUDGED cells of (r, j):
 *   inFinal == 0: the offsets max(0, last - d_r) <= o <= last - 1 -- the cells whose entry ends inside the d_r sub-fingerprints in
 *                 front of the newest one; none when d_r == 0 or last == 0;
 *   inFinal != 0: max(0, last - d_r) <= o <= last -- the newest cell too; d_r == 0 gives the newest cell alone.  For the end of a
 *                 stream, or before a channel is reset.
 * A judged cell matches when q_o >= inThreshold as Float32, (o == 0 or q_o > q_(o-1)) and (o == last or q_o >= q_(o+1)), q the
 * window's own LBAudioDetectiveCorpusMatchProfile values bit for bit: exactly the occurrences call's rule -- a plateau reports its
 * first cell, and a neighbour below the threshold still takes part in the test.
 * Row r is, bit for bit, row r of LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice with inPeaksOnly = 1 and the same other
 * arguments with only the judged cells kept: the key format, lags -o, (entry ascending, offset ascending) order, zero keys and lags
 * 0 behind min(count, inCapacity), the TRUE count in outCounts[r], nothing written next door on overflow, nothing of recording
 * r +- 1 in a cell of r.  Shards merge per recording by concatenation.
 * ONCE IN A CHANNEL'S LIFE: feed a channel in pushes d_1, d_2, ..., each at most inMaxNew; call with inFinal = 0 after each push,
 * on a window that holds the channel's whole life so far or is at least (longest entry + d_k + 1) long -- TWO sub-fingerprints more
 * than the peak-less call needs: the cell judged furthest back and its left neighbour --; make one last call with inFinal = 1 and
 * new count 0 on the final window.  Moved to absolute positions (total - inSubfingerprints + o), the cells of all calls together
 * are the cells of ONE occurrences call with peaks on over the whole recording, for the entries not longer than the windows: each
 * appears exactly once, with equal key bits.
 * Refusals in the tail call's order and with its codes; inMaxNew is refused at 0 or above 62.  An empty corpus, or no entry that
 * takes part, is noErr with zero keys, lags and counts.
 * Asynchronous on inStream, which it never awaits; it waits ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * Results do not depend on launch order, grid, passes, chunks or outLags, nor on inMaxNew beyond the clamp.  Nothing is carried
 * from call to call: a pair computes d_r + 2 cells (k_occurrences_tail.hip).
 * LBAudioDetectiveDebugOccurrencesTailPeaksPlan: the call's plan, arguments and outputs as LBAudioDetectiveDebugOccurrencesTailPlan
 * -- it IS that plan at inMaxNew + 2 (D the next power of two >= inMaxNew + 2), from the same function as the call's. */
#define LBAD_OCCURRENCES_TAIL_PEAKS_MAX_NEW 62
OSStatus LBAudioDetectiveCorpusQueryPackedOccurrencesTailPeaksBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus,
                                                                              const void* inPackedQueries, UInt32 inRecordings,
                                                                              UInt32 inSubfingerprints, const void* inNewCounts,
                                                                              UInt32 inMaxNew, UInt32 inFinal, UInt32 inRange,
                                                                              Float32 inThreshold, UInt64 inCapacity, UInt64 inIndexBase,
                                                                              void* outKeys, void* outLags, void* outCounts,
                                                                              void* inStream);
OSStatus LBAudioDetectiveDebugOccurrencesTailPeaksPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry,
                                                       UInt32 inLongestEntry, UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit,
                                                       UInt32* outLanes, UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords,
                                                       UInt64* outLdsBytes, UInt32* outRecordingsPerPass, UInt64* outEntriesPerChunk,
                                                       UInt64* outScratchBytes);
/* Live best matches: the cells of the tail occurrences call above folded to ONE value per (recording, entry) -- which entries a
 * push completed on each channel, as per-entry scores, as the K best, or as all at or above a score -- in a fixed output shape.
 * Cells, d_r, the entries that take part and a cell's value are EXACTLY those of
 * LBAudioDetectiveCorpusQueryPackedOccurrencesTailBatchKeysDevice; inPackedQueries, inRecordings, inSubfingerprints, inNewCounts
 * (DEVICE, UInt32 [inRecordings], 4-byte aligned), inMaxNew (1 .. LBAD_OCCURRENCES_TAIL_MAX_NEW), inRange and inStream are its.  For
 * recording r and entry j:
 *   score[r][j] = max(+0, the largest q_o over the tail cells of (r, j)) as Float32; +0 when the pair has no tail cell (d_r == 0,
 *                 n_j == 0, or n_j > inSubfingerprints);
 *   lag[r][j]   = -(the LOWEST tail offset whose q_o equals the score); 0 when no tail cell equals it.
 * ...RecordingPackedScoresTailBatchDevice writes both as [inRecordings][entries] on the device (outLags may be NULL); every word
 * is written, an empty corpus writes nothing; inRecordings x entries <= 2^31 - 1.
 * ...QueryPackedRecordingTopKTailBatchKeysDevice: outKeys [inRecordings][inK] UInt64, outLags the same shape SInt32 or NULL.  Row r
 * is the batch recording top-K's selection over row r of the scores: the entries with score > 0, keys score bits << 32 | 0xFFFFFFFF
 * - (inIndexBase + j) descending (so the lowest index first among equal scores), zero keys behind them, each key's lag beside
 * it and lag 0 for a zero key.  1 <= inK <= LBAD_TOPK_MAX, inRecordings x inK <= 2^31.
 * ...QueryPackedRecordingThresholdTailBatchKeysDevice: outKeys [inRecordings][inCapacity], outCounts UInt64 [inRecordings], outLags
 * or NULL.  Row r is the batch recording threshold's selection over row r of the scores: the entries with score >= inThreshold
 * in ascending index, outCounts[r] the TRUE count, zero keys behind min(count, inCapacity), lag 0 for a zero key.  Threshold
 * (finite, > 0) and capacity (1 .. 2^31, inRecordings x inCapacity <= 2^31) are the batch call's.
 * What follows from this:
 * EQUIVALENCE with the tail occurrences call: the threshold call's row r names exactly the DISTINCT entries of row r of the tail
 * occurrences call at the same threshold (while that row is not cut), each with the key of its largest cell and the lag of the
 * lowest offset that reaches it.
 * ONCE PER PUSH: a (channel, entry) pair is reported at most once per push, and only by the push that completes its best new
 * cell.  Under the tail occurrences' window condition (window >= longest entry + d_k - 1) the union over a channel's pushes of
 * (entry, absolute start = total - inSubfingerprints - lag) is a subset of the whole recording's occurrences' cells and holds, for
 * every push and entry, that push's best cell.
 * INDEPENDENCE: results do not depend on launch order, grid, passes, outLags, or inMaxNew beyond the clamp.
 * Refusals in the tail occurrences call's order: what needs no handle first (a NULL pointer other than outLags, inNewCounts not
 * 4-byte aligned, inMaxNew 0 or above the cap, inK, inThreshold, inCapacity, inIndexBase and the products above), then
 * kLBAudioDetectiveDeviceUnavailable, then what needs the corpus (as the tail occurrences call).  An empty corpus, or one with no
 * entry that takes part, is noErr with zero keys, lags and counts; the scores form writes +0 scores and 0 lags when entries exist
 * but none takes part.
 * Asynchronous on inStream, which they never await; they wait ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * One compute launch per pass (k_recording_tail.hip: no counts, no scans, no scatter), then the selection.
 * LBAudioDetectiveDebugRecordingTailPlan is the calls' plan on the host -- they take theirs from the same function --; it needs
 * neither device nor handle: the lanes per recording, the recordings per workgroup, the records of a recording's LDS window and
 * the LDS of a workgroup exactly as LBAudioDetectiveDebugOccurrencesTailPlan gives them; the recordings per pass -- all entries
 * in one launch, at most 65 535 recordings, blocks of 64 entries x recordings within 32 bits, and with inKeyForm != 0 at most
 * max(1, limit / (entries x 8)), the score and lag rows the selection reads (inScratchLimit 0: the default) --; and the scratch
 * of a pass (those rows: recordings per pass x entries x 8 bytes; 0 without inKeyForm).  kLBAudioDetectiveArgumentInvalid for a
 * shape the call refuses or a NULL pointer. */
OSStatus LBAudioDetectiveCorpusRecordingPackedScoresTailBatchDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                    UInt32 inRecordings, UInt32 inSubfingerprints, const void* inNewCounts,
                                                                    UInt32 inMaxNew, UInt32 inRange, Float32* outScores, SInt32* outLags,
                                                                    void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedRecordingTopKTailBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                           UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                           const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                           UInt32 inK, UInt64 inIndexBase, void* outKeys, void* outLags,
                                                                           void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedRecordingThresholdTailBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus,
                                                                                const void* inPackedQueries, UInt32 inRecordings,
                                                                                UInt32 inSubfingerprints, const void* inNewCounts,
                                                                                UInt32 inMaxNew, UInt32 inRange, Float32 inThreshold,
                                                                                UInt64 inCapacity, UInt64 inIndexBase, void* outKeys,
                                                                                void* outCounts, void* outLags, void* inStream);
OSStatus LBAudioDetectiveDebugRecordingTailPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inLongestEntry, UInt64 inEntries,
                                                UInt32 inMaxNew, UInt64 inScratchLimit, UInt32 inKeyForm, UInt32* outLanes,
                                                UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords, UInt64* outLdsBytes,
                                                UInt32* outRecordingsPerPass, UInt64* outScratchBytes);
/* Live timeline: every channel's timeline kept current from each push.  A cell's value depends only on the entry and the
 * sub-fingerprints under it, so the timeline of a window after a push is the previous timeline shifted left by the push's count,
 * merged by element-wise UNSIGNED maximum with the cells the push completed; no window-length condition applies and nothing is
 * computed again.  inPackedQueries ([inRecordings][n][32] bytes, n = inSubfingerprints: the windows AFTER the push, as
 * LBAudioDetectiveStreamBankWindowDevice writes them), inNewCounts (DEVICE, UInt32 [inRecordings], 4-byte aligned, read on the
 * stream), inMaxNew (1 .. LBAD_OCCURRENCES_TAIL_MAX_NEW), inRange and inStream are the tail occurrences call's; inThreshold (finite,
 * > 0) and inIndexBase are the batch timeline's.  inPrevKeys (may be NULL) and outKeys are UInt64 [inRecordings][n], outLengths
 * (may be NULL) UInt32 [inRecordings][n], all on the device.  With shift_r = min(inNewCounts[r], n) and cells_r =
 * min(inNewCounts[r], inMaxNew, n):
 *   T_r[o] = the unsigned maximum of  q_o(j) bits << 32 | 0xFFFFFFFF - (inIndexBase + j)  over the tail occurrences call's cells of
 *            (r, j) at cells_r that reach inThreshold -- the entries with 1 <= n_j <= n at the offsets max(0, n - n_j - cells_r + 1)
 *            <= o <= n - n_j, q_o as LBAudioDetectiveCorpusMatchProfile gives it --, 0 where none does;
 *   P_r[o] = inPrevKeys[r][o + shift_r] while o + shift_r < n, else 0; 0 everywhere when inPrevKeys is NULL;
 *   outKeys[r][o] = max(T_r[o], P_r[o]);
 *   outLengths[r][o] = n_j of the entry the key names, looked up in the corpus: 0 for a zero key or an index outside the corpus.
 * Every word of both outputs is written.  With inPrevKeys == NULL row r is the batch timeline's row r with only the tail cells
 * counting: the form shards exchange, and shards merge by element-wise unsigned maximum as the timeline's do.
 * INVARIANT: seed inPrevKeys with LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice on a channel's window; after every
 * push whose new count is <= inMaxNew call this with the new window and the previous output.  Then outKeys and outLengths equal,
 * bit for bit, what the batch timeline call writes for the new window -- for the same corpus contents, threshold, range and index
 * base; ties go to the lowest index as there.  A count ABOVE inMaxNew still shifts by the true count but adds only the newest
 * inMaxNew cells: the row then lacks the cells in between until they have slid out of the window (seed again instead).  The
 * caller also seeds again after entries were removed from the corpus or a channel was reset; the state is the caller's two
 * buffers, nothing is kept in the corpus.
 * INDEPENDENCE: results do not depend on grid, launch order, passes, outLengths, or inMaxNew beyond the clamp.
 * Refusals in the tail calls' order: what needs no handle first (a NULL pointer other than inPrevKeys and outLengths, inNewCounts
 * not 4-byte aligned, inMaxNew 0 or above the cap, inThreshold, inIndexBase > 2^32, inRecordings x n > 2^31 - 1, and [inPrevKeys,
 * + inRecordings x n x 8) overlapping [outKeys, + inRecordings x n x 8)), then kLBAudioDetectiveDeviceUnavailable, then what needs
 * the corpus (not ragged, an entry above LBAD_OCCURRENCES_MAX_ENTRY_SUBFINGERPRINTS, inIndexBase + entries > 2^32, a join scratch
 * limit that holds no strip of one recording).  An empty corpus, or one with no entry that takes part, is noErr with the shifted
 * previous rows and lengths looked up as above -- zeros without inPrevKeys.
 * Asynchronous on inStream, which it never awaits; it waits ON THE DEVICE for the corpus' latest append; nothing visits the host.
 * Per pass of recordings: the strips zeroed, one compute launch over all entries, one finishing launch (k_timeline_tail.hip).
 * LBAudioDetectiveDebugTimelineTailPlan is the call's plan on the host -- it takes its own from the same function --; it needs
 * neither device nor handle: the lanes per recording and the records of a recording's LDS window as
 * LBAudioDetectiveDebugOccurrencesTailPlan gives them; the strip width min(longest entry, n) - shortest entry + lanes (0 where no
 * entry takes part); the recordings per workgroup -- 256 / lanes, fewer where that many windows (36 bytes a record) and strips (8
 * bytes a slot) with the table do not fit 160 KiB - 64 --; the LDS of a workgroup; the recordings per pass -- at most 65 535,
 * blocks of 64 entries x recordings within 32 bits, and limit / (strip width x 8) (inScratchLimit 0: the default) --; and the
 * scratch of a pass (recordings per pass x strip width x 8 bytes).  kLBAudioDetectiveArgumentInvalid for a shape the call refuses,
 * a limit below one strip, or a NULL pointer. */
OSStatus LBAudioDetectiveCorpusRecordingPackedTimelineTailBatchKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                                          UInt32 inRecordings, UInt32 inSubfingerprints,
                                                                          const void* inNewCounts, UInt32 inMaxNew, UInt32 inRange,
                                                                          Float32 inThreshold, UInt64 inIndexBase,
                                                                          const void* inPrevKeys /* may be NULL */, void* outKeys,
                                                                          void* outLengths /* may be NULL */, void* inStream);
OSStatus LBAudioDetectiveDebugTimelineTailPlan(UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inShortestEntry, UInt32 inLongestEntry,
                                               UInt64 inEntries, UInt32 inMaxNew, UInt64 inScratchLimit, UInt32* outLanes,
                                               UInt32* outRecordingsPerWorkgroup, UInt32* outWindowRecords, UInt32* outStripWidth,
                                               UInt64* outLdsBytes, UInt32* outRecordingsPerPass, UInt64* outScratchBytes);
/* Recording segments: "what played when" from a timeline's per-offset winners, on the device -- non-overlapping spans per
 * recording, for one recording (inRecordings == 1) or a batch.  inKeys ([inRecordings][inSubfingerprints] UInt64) and inLengths
 * (the same shape, UInt32) are what LBAudioDetectiveCorpusRecordingPackedTimelineBatchKeysDevice or the single timeline calls
 * write, or the element-wise maximum of several shards' keys with the winners' lengths.  Independently per recording r: the
 * candidates are the offsets o with a non-zero key AND a non-zero length; they are visited in descending 64-bit key order (higher
 * score bits, then lower entry index), equal keys at the lower offset first, and a candidate is accepted when
 * [o, min(o + length, inSubfingerprints)) meets no span accepted before it -- spans that only touch do not meet, and nothing of
 * another recording ever blocks an offset.  This is what timeline_segments of the Python interface computes on the host.
 * Row r of outStarts / outKeys / outLengths ([inRecordings][inCapacity]; outLengths may be NULL and changes nothing else) holds
 * the accepted spans in ascending start order in slots 0 .. min(count, inCapacity) - 1: the start, the key UNCHANGED -- so
 * LBAudioDetectiveCorpusIdsFromKeysDevice, ...GatherKeysDevice, ...AlignKeysDevice and ...RemoveKeysDevice read outKeys as it is
 * -- and the length as inLengths holds it; zeros stand behind them and every word of every row is written.  outCounts[r] is the
 * TRUE number of spans, never cut; above inCapacity the row holds the first inCapacity spans by start.
 * The call takes no handle and needs no scratch: one launch (k_segments.hip: a workgroup per recording, its state in
 * 10 x n2 + 2.25 x inSubfingerprints bytes of LDS and a little, n2 the power of two >= max(inSubfingerprints, 64) -- 100 872
 * bytes at the cap, which is what LBAD_SEGMENTS_MAX_SUBFINGERPRINTS comes from), asynchronous on
 * inStream, which it never awaits.  Results do not depend on grid, launch order, stream or outLengths.  The outputs must overlap
 * no input.
 * Refusals, each kLBAudioDetectiveArgumentInvalid and decided before anything touches a device: a NULL pointer other than
 * outLengths; inRecordings, inSubfingerprints or inCapacity 0; inSubfingerprints > LBAD_SEGMENTS_MAX_SUBFINGERPRINTS;
 * inRecordings x inSubfingerprints or inRecordings x inCapacity above 2^31 - 1; a pointer not aligned to its element (8 bytes for
 * the key blocks, 4 for the others); outKeys == inKeys or outLengths == inLengths.  Then a missing device is
 * kLBAudioDetectiveDeviceUnavailable. */
#define LBAD_SEGMENTS_MAX_SUBFINGERPRINTS 8192
OSStatus LBAudioDetectiveTimelineSegmentsFromKeysDevice(const void* inKeys /* device, [inRecordings][inSubfingerprints] UInt64 */,
                                                        const void* inLengths /* device, same shape, UInt32 */,
                                                        UInt32 inRecordings, UInt32 inSubfingerprints, UInt32 inCapacity,
                                                        void* outStarts /* device, [inRecordings][inCapacity] UInt32 */,
                                                        void* outKeys /* device, [inRecordings][inCapacity] UInt64 */,
                                                        void* outLengths /* device, [inRecordings][inCapacity] UInt32, may be NULL */,
                                                        void* outCounts /* device, [inRecordings] UInt32 */, void* inStream);
/* Occurrence segments: "what played when" over ALL matching cells, on the device -- the call above sees one candidate per offset
 * (the timeline's winner) and so never reports the second best entry at an offset, even where the winner there loses to a better
 * overlapping span; this call runs the same greedy over the rows of an occurrences call, where any number of entries may start
 * at one offset.  inKeys / inLags ([inRecordings][inCapacity] UInt64 / SInt32) are what
 * LBAudioDetectiveCorpusQueryPackedOccurrencesBatchKeysDevice or the single occurrences calls write (with inPeaksOnly one cell per
 * airing), inLengths (same shape, UInt32) the sub-fingerprints of the entry each key names, as
 * LBAudioDetectiveCorpusEntryLengthsFromKeysDevice (below) writes them, inCounts ([inRecordings] UInt64, may be NULL) the
 * occurrences calls' counts.  Shards concatenate their rows, each with the lengths of its own keys, and pass inCounts NULL: zero
 * keys between the shards' cells are no candidates.
 * Independently per recording r.  The slots p < m are considered, m = min(inCounts[r], inCapacity), or inCapacity without
 * inCounts; non-zero keys behind m are ignored.  A slot is a candidate when its key is non-zero, its length is non-zero and its
 * span [s, e) is not empty: s = max(0, -lag), e = min(inSubfingerprints, -lag + length), in 64-bit signed arithmetic (any lag
 * word is harmless), with s < inSubfingerprints and s < e.  With the occurrences' lag convention lag = -o places the entry at
 * offset o of the recording, and lag = +o says that the recording lies inside a longer entry, which then spans the whole
 * recording.  The candidates are visited in descending 64-bit key order (higher score bits, then lower entry index), equal keys
 * at the lower s first, equal keys and s at the lower slot first, and a candidate is accepted when its span meets no span
 * accepted before it -- spans that only touch do not meet, and nothing of another recording ever blocks an offset.  This is what
 * occurrence_segments of the Python interface computes on the host.
 * Row r of outStarts / outKeys / outLags / outLengths ([inRecordings][inOutCapacity]; outLags and outLengths may each be NULL and
 * change nothing else) holds the accepted spans in ascending start order in slots 0 .. min(count, inOutCapacity) - 1: s, then
 * key, lag and length UNCHANGED -- so LBAudioDetectiveCorpusIdsFromKeysDevice, ...GatherKeysDevice, ...AlignKeysDevice and
 * ...RemoveKeysDevice read outKeys as it is; accepted spans do not overlap, so the starts are distinct.  Zeros stand behind them
 * and every word of every row is written.  outCounts[r] is the TRUE number of spans, never cut.  A row of the occurrences call
 * that overflowed (its count above inCapacity) was cut in (entry, offset) order before this greedy ran: raise the capacity or the
 * threshold, or ask for peaks only.
 * The call takes no handle and needs no scratch: one launch (k_occurrence_segments.hip: a workgroup per recording, its state in
 * 14 x n2 + 2.25 x inSubfingerprints bytes of LDS and a little, n2 the power of two >= max(inCapacity, 64) -- 133 640 bytes at
 * both caps), asynchronous on inStream, which it never awaits.  Results do not depend on grid, launch order, stream or which of
 * the optional outputs are NULL.  The outputs must overlap no input.
 * Refusals, each kLBAudioDetectiveArgumentInvalid and decided before anything touches a device: a NULL pointer other than
 * inCounts, outLags or outLengths; inRecordings, inCapacity, inSubfingerprints or inOutCapacity 0; inSubfingerprints >
 * LBAD_SEGMENTS_MAX_SUBFINGERPRINTS; inCapacity > LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES; inRecordings x inCapacity,
 * inRecordings x inSubfingerprints or inRecordings x inOutCapacity above 2^31 - 1; a pointer not aligned to its element (8 bytes
 * for the key blocks and inCounts, 4 for the others); outKeys == inKeys, outLags == inLags or outLengths == inLengths.  Then a
 * missing device is kLBAudioDetectiveDeviceUnavailable.
 * LBAudioDetectiveCorpusEntryLengthsFromKeysDevice: outLengths[i] (UInt32, device) = the sub-fingerprints of the entry inKeys[i]
 * names (the low word is 0xFFFFFFFF - (inIndexBase + index), the score word is ignored), 0 for a zero key and for an index
 * outside [inIndexBase, inIndexBase + entries) -- a ragged corpus' own entry lengths, a uniform corpus' one length.  A shard
 * serves exactly the keys of its own range.  1 <= inCount <= 2^31 - 1; asynchronous on inStream, which it never awaits; it waits
 * ON THE DEVICE for the corpus' latest append, and like every other call it must not run concurrently with a removal.  A NULL
 * handle or pointer, inCount 0 or above 2^31 - 1, inIndexBase > 2^32 and a pointer not aligned to its element are
 * kLBAudioDetectiveArgumentInvalid, decided before a handle is read; then a missing device is
 * kLBAudioDetectiveDeviceUnavailable; then inIndexBase + entries > 2^32 is kLBAudioDetectiveArgumentInvalid. */
#define LBAD_OCCURRENCE_SEGMENTS_MAX_CANDIDATES 8192
OSStatus LBAudioDetectiveOccurrenceSegmentsFromKeysDevice(const void* inKeys /* device, [inRecordings][inCapacity] UInt64 */,
                                                          const void* inLags /* device, same shape, SInt32 */,
                                                          const void* inLengths /* device, same shape, UInt32 */,
                                                          const void* inCounts /* device, [inRecordings] UInt64, may be NULL */,
                                                          UInt32 inRecordings, UInt32 inCapacity, UInt32 inSubfingerprints,
                                                          UInt32 inOutCapacity,
                                                          void* outStarts /* device, [inRecordings][inOutCapacity] UInt32 */,
                                                          void* outKeys /* device, same shape, UInt64 */,
                                                          void* outLags /* device, same shape, SInt32, may be NULL */,
                                                          void* outLengths /* device, same shape, UInt32, may be NULL */,
                                                          void* outCounts /* device, [inRecordings] UInt32 */, void* inStream);
OSStatus LBAudioDetectiveCorpusEntryLengthsFromKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys /* device */,
                                                          UInt64 inCount, UInt64 inIndexBase, void* outLengths /* device */,
                                                          void* inStream);
/* Removal: entries taken out of a corpus on the device, the other half of the corpus life cycle -- the take-down of one
 * recording, or the action behind a join's duplicate pairs.  Both forms, both kinds of corpus (uniform of any shape, ragged):
 * the named entries go, the others keep their relative order and close up -- the entry at old index i gets the new index
 * i - (removed entries below i).  Afterwards the corpus cannot be told from one made fresh with the same capacities by
 * appending the kept entries in order: every query form returns the same bits, LBAudioDetectiveCorpusSave writes the same
 * bytes, GetCount and GetSubfingerprintTotal return the same values.  Capacity and the addresses of the corpus' blocks do not
 * change; later appends reuse the room that was freed.  outRemoved receives the number of DISTINCT entries removed (0 from a
 * call that is refused or fails, wherever outRemoved itself is not NULL);
 * outNewIndices, when given, one UInt32 per OLD entry: its new index, or 0xFFFFFFFF for a removed entry.
 * LBAudioDetectiveCorpusRemoveIndices takes indices on the host (outNewIndices: host).  Duplicates are allowed; any index >= the
 * count is kLBAudioDetectiveArgumentInvalid and nothing changes.
 * LBAudioDetectiveCorpusRemoveKeysDevice takes inCount 64-bit keys on the device exactly as the top-K, threshold and join calls
 * write them -- the low word is 0xFFFFFFFF - (inIndexBase + index), the score word is ignored -- and outNewIndices is a device
 * pointer.  Zero keys and keys whose index lies outside [inIndexBase, inIndexBase + count) are skipped (the alignment's
 * convention), duplicates are allowed: a key list padded with zeros can be passed as it is.  Its kernels run on inStream, the
 * stream that produced the keys (or one the caller has put behind their producer).
 * A removal is a SYNCHRONOUS maintenance call: it first waits for everything the corpus has in flight (appends, queries of
 * every form, alignments, joins), and both forms return when the device work is done and the count (and a ragged corpus'
 * offsets and length histogram) are up to date; everything issued later finds the new corpus.  One read-back per call: the
 * tile offsets, and the index map when the host form returns it or the corpus is ragged.  Like appends, a removal must not run
 * concurrently with any other call on the same corpus.  The sharded key block is left alone; a sharded corpus has no removal
 * by index (the index bases of all later shards would shift) -- with entry ids each rank takes down by id on its own (below).
 * inCount == 0, or a list that names nothing valid: noErr, 0 removed, the identity map, nothing is moved.  Removing every entry
 * leaves a working empty corpus; removing only the last entries moves nothing (entries below the lowest removed index are
 * neither read nor written).  A NULL handle, a NULL outRemoved, a NULL list with inCount != 0 and inIndexBase > 2^32 are
 * kLBAudioDetectiveArgumentInvalid, decided before a handle is read; then a missing device is
 * kLBAudioDetectiveDeviceUnavailable; then inIndexBase + count > 2^32 is kLBAudioDetectiveArgumentInvalid.
 * The scratch belongs to the corpus and grows on demand: the index block, 4 x (8 + 2 x tiles + 2 x 1024 x tiles) + 4 bytes
 * rounded up to 16 for tiles = ceil(count / 1024) tiles of 1024 entries (flags, map, tile counts and offsets); the host form's
 * staged list, 8 x inCount bytes; a ragged corpus' second offsets array, 4 x (entry capacity + 1) bytes; and the bounce buffer
 * the kept planes or records pass through in ascending chunks, min(limit, items above the lowest removed index rounded up to
 * whole tiles) x LBAudioDetectiveCorpusGetEntryStrideBytes, a whole number of tiles of 1024 entries (uniform) or 1024 records
 * (ragged).  LBAudioDetectiveCorpusSetRemoveScratchLimit bounds the bounce buffer (0 = the default, 256 MiB) and so sets the
 * items per chunk; a limit below one tile is kLBAudioDetectiveArgumentInvalid at the removal call, and the result never depends
 * on the limit. */
OSStatus LBAudioDetectiveCorpusRemoveIndices(LBAudioDetectiveCorpusRef inCorpus, const UInt64* inIndices, UInt64 inCount,
                                             UInt32* outNewIndices /* host, may be NULL */, UInt64* outRemoved);
OSStatus LBAudioDetectiveCorpusRemoveKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys /* device */, UInt64 inCount,
                                                UInt64 inIndexBase, void* outNewIndices /* device, may be NULL */,
                                                UInt64* outRemoved /* host */, void* inStream);
OSStatus LBAudioDetectiveCorpusSetRemoveScratchLimit(LBAudioDetectiveCorpusRef inCorpus, UInt64 inBytes);   /* 0 = default */
/* Gather: entries handed back out of a corpus on the device, in the packed layout LBAudioDetectiveFingerprintClipsDevice writes
 * and every ...Packed...Device query and both Append...PackedDevice calls read -- so the matches of a top-K, threshold or join
 * call can be queried again (also against a ragged corpus, with its own entries), appended to another corpus or looked at,
 * without the host seeing them.  Both kinds of corpus (uniform of any shape, ragged).
 * Rows and offsets.  Row i of the output belongs to element i of the list, in list order; nothing is sorted, a duplicate yields
 * a second copy.  LBAudioDetectiveCorpusGatherKeysDevice reads inCount 64-bit keys on the device as
 * LBAudioDetectiveCorpusRemoveKeysDevice reads them: the low word is 0xFFFFFFFF - (inIndexBase + index), the score word is
 * ignored.  A zero key, or a key whose index lies outside [inIndexBase, inIndexBase + count), yields an EMPTY row (the
 * alignment's and the removal's convention): a top-K or threshold row padded with zeros can be passed as it is.  outOffsets
 * receives inCount + 1 UInt64: offsets[0] = 0, offsets[i + 1] - offsets[i] = the sub-fingerprints of row i (0 for an empty row,
 * subfingerprintsPerEntry for a uniform corpus, the entry's own count for a ragged one), offsets[inCount] = the TRUE total,
 * never cut.
 * Packed output and capacity.  outPacked has room for inCapacity sub-fingerprints of LBAD_PACKED_BYTES each.  The sub-fingerprint
 * at output position p (row i's sub-fingerprint s at offsets[i] + s) is written when p < inCapacity; nothing is written at or
 * beyond the capacity.  A total above the capacity tells that the output was cut, which is no error; an entry may be cut in
 * the middle.  inCapacity == 0 with outPacked == NULL is the sizing call: it writes the offsets only.
 * Bytes returned.  Boolean b at bit b & 31 of word b >> 5.  The output holds the stored Booleans below the sub-fingerprint
 * length rounded up to an even number -- what both corpus layouts keep -- and every higher bit is zero; the derived fields of a
 * ragged corpus' records never appear.  For rows that were appended with their unused bits zero (the packed contract) the
 * gather returns the appended bytes bit for bit, and appending a gathered entry to a fresh corpus reproduces its stored bytes.
 * Sharding.  A shard with inIndexBase serves exactly the keys of its own range and leaves the other rows empty; the outputs of
 * all ranks for one key list merge by taking, per row, the one non-empty copy.
 * The device form writes to device pointers (outPacked 16-byte aligned, inKeys and outOffsets 8-byte aligned; anything else is
 * kLBAudioDetectiveArgumentInvalid), asynchronously on inStream, which it never awaits; it waits ON THE DEVICE for the latest
 * append.  The scratch belongs to the corpus: 8 x ceil(inCount / 1024) bytes, the sums of the tiles of 1024 keys (the row
 * lengths themselves are scanned in place in outOffsets).  It grows on demand, and a call waits for the previous gather's device
 * work before it reuses it.  Like every other call, a gather must not run concurrently with a removal of the same corpus.
 * LBAudioDetectiveCorpusGatherIndices is the device form on the null stream with one read-back: indices, packed bytes and
 * offsets are in host memory, duplicates are allowed, and any index >= the count is kLBAudioDetectiveArgumentInvalid with
 * nothing written.
 * LBAudioDetectiveCorpusCopyFingerprint returns a NEW host fingerprint holding entry inIndex -- the corpus' sub-fingerprint
 * length, the entry's sub-fingerprints in order; it equals (LBAudioDetectiveFingerprintEqualToFingerprint) the fingerprint
 * LBAudioDetectiveCorpusAppendFingerprint stored, and the caller disposes it.  NULL for a NULL corpus, an index >= the count,
 * no device or a failed device call.
 * A NULL corpus, a NULL outOffsets, a NULL list with inCount != 0, a NULL outPacked with inCapacity != 0, inCount > 2^31 and
 * inIndexBase > 2^32 are kLBAudioDetectiveArgumentInvalid, decided before a handle is read; then a missing device is
 * kLBAudioDetectiveDeviceUnavailable; then inIndexBase + entries > 2^32 is kLBAudioDetectiveArgumentInvalid.  inCount == 0 is
 * noErr and writes offsets[0] = 0; an empty corpus makes every row empty. */
OSStatus LBAudioDetectiveCorpusGatherKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys /* device */,
                                                UInt64 inCount, UInt64 inIndexBase, void* outPacked /* device */,
                                                UInt64 inCapacity, void* outOffsets /* device */, void* inStream);
OSStatus LBAudioDetectiveCorpusGatherIndices(LBAudioDetectiveCorpusRef inCorpus, const UInt64* inIndices, UInt64 inCount,
                                             void* outPacked /* host */, UInt64 inCapacity, UInt64* outOffsets /* host */);
LBAudioDetectiveFingerprintRef LBAudioDetectiveCorpusCopyFingerprint(LBAudioDetectiveCorpusRef inCorpus, UInt64 inIndex);
/* Entry ids: the caller's own 64-bit id of every entry, kept on the device with the entry.  Every result names an entry by its
 * index, and a removal gives every later entry a new index; an id stays with its entry through removals, is stored by
 * LBAudioDetectiveCorpusSave, comes back for any match (IdsFromKeys) and names the entries of a take-down or a hand-back
 * (KeysFromIds, whose output RemoveKeysDevice, GatherKeysDevice and AlignKeysDevice take as it is).  Both kinds of corpus.
 * Model.  A corpus either has ids or it has none; it starts without.  The first successful SetEntryIds... call with a
 * non-empty range turns ids on: `capacity` UInt64 on the device, all zero, a block that never moves.  Id 0 means "no id".  The
 * words at and above the count are always zero, so appended entries have id 0 until the caller sets them, and no append knows of
 * ids.  Duplicate ids are legal; wherever an id has to name ONE entry, the LOWEST index wins.  Ids are global by nature:
 * inIndexBase applies to keys only.  A corpus that never sets an id gets no new memory, launches nothing new and writes the same
 * file bytes as before.
 * SetEntryIdsDevice / SetEntryIds: entries [inFirst, inFirst + inCount) get the inCount ids at inIds (device, 8-byte aligned / host).
 * inFirst + inCount > count is kLBAudioDetectiveArgumentInvalid and nothing changes; inCount == 0 is noErr and does NOT turn ids
 * on.  The device form is asynchronous on inStream.  The host form copies the ids into pinned staging of the corpus (8 x inCount
 * bytes, grown on demand) and returns when the copy from there is enqueued on the null stream: inIds may be reused at once.
 * GetEntryIds: a synchronous read-back of the words [inFirst, inFirst + inCount) to host memory; the range may reach up to the
 * CAPACITY (the words from the count on read as zero, which is the invariant above), beyond it kLBAudioDetectiveArgumentInvalid.
 * A corpus without ids gives zeros.  HasEntryIds: 1 for a corpus with ids, else 0 (also for NULL); needs no device.
 * IdsFromKeysDevice: inCount 64-bit keys on the device, read exactly as RemoveKeysDevice and GatherKeysDevice read them (the low
 * word is 0xFFFFFFFF - (inIndexBase + index), the score word is ignored) -> outIds[i], the id of the entry key i names; 0 for a
 * zero key, for an index outside [inIndexBase, inIndexBase + count), or for a corpus without ids.  All inCount words are
 * written, nothing behind them.  It serves the key block of every call that writes this key format: top-K, threshold, the packed
 * forms, both joins, occurrences, the recording forms, the timeline, the groups' extra keys.  One launch (a corpus without ids:
 * one memset and no allocation).
 * KeysFromIdsDevice: inCount ids on the device -> outKeys[i] = bits(1.0f) << 32 | 0xFFFFFFFF - (inIndexBase + index) for the
 * LOWEST index whose id equals inIds[i] -- LBAudioDetectiveGroupExtraKeysFromLabelsDevice's convention, a key is never zero by
 * accident -- and the zero key for id 0, an id no entry has, or a corpus without ids.  List order, duplicates allowed.  The
 * lookup goes through an index on the device: an open-addressing table of slots = the power of two >= 2 x count (at least 1024),
 * 12 bytes a slot, built whole (two launches) on the call's stream by the first KeysFromIds after anything made it stale -- ids
 * set, a removal, a load; an append alone does not -- and kept until it is stale again or the corpus is disposed.
 * Removal.  Both removal calls move the ids of a corpus that has them with the SAME device map as the entries, through a block
 * of its own of 8 x (count - lowest removed index) bytes (two launches; the result never depends on
 * LBAudioDetectiveCorpusSetRemoveScratchLimit), zero the words from the new count to the old one, and make the index stale.
 * Save / Load.  A corpus with ids writes a trailer behind the payload of either file kind: "LBADIDS1", UInt64 count, count x
 * UInt64.  Load of such a file turns ids on; the trailer is untrusted: a count other than the payload's, or fewer bytes than
 * announced, make Load return NULL.  Bytes behind a payload that do not start with the magic are ignored, as before.
 * Refusals, in this order.  Decided before a handle is read, each kLBAudioDetectiveArgumentInvalid: a NULL corpus; a NULL pointer
 * with inCount != 0; a device pointer not aligned to 8 bytes; inIndexBase > 2^32; inCount > 2^31 (the list calls) or inFirst or
 * inCount > 2^32 (the range calls).  Then a missing device is kLBAudioDetectiveDeviceUnavailable.  Then what needs the corpus,
 * kLBAudioDetectiveArgumentInvalid: inIndexBase + count > 2^32, the range rules of Set and Get.  Then inCount == 0 is noErr.  A
 * refused call reserves nothing, launches nothing and touches no event.
 * Asynchrony.  One event of the corpus covers the id block, the index, the removal's block and the staging: every id call waits
 * for the previous id call's device work before it touches any of them and records the event behind its last launch, also
 * after a failure.  IdsFromKeysDevice and KeysFromIdsDevice never await inStream and read nothing back; they wait ON THE DEVICE
 * for the latest append, as the gather does.  A removal and LBAudioDetectiveCorpusDispose await the event.  Like every other
 * call, none of these may run concurrently with a removal of the same corpus.  LBAudioDetectiveCorpusGather...'s packed output
 * carries no ids: IdsFromKeysDevice with the same key list gives them. */
OSStatus LBAudioDetectiveCorpusSetEntryIdsDevice(LBAudioDetectiveCorpusRef inCorpus, UInt64 inFirst, UInt64 inCount,
                                                 const void* inIds /* device, 8-byte aligned */, void* inStream);
OSStatus LBAudioDetectiveCorpusSetEntryIds(LBAudioDetectiveCorpusRef inCorpus, UInt64 inFirst, UInt64 inCount, const UInt64* inIds /* host */);
OSStatus LBAudioDetectiveCorpusGetEntryIds(LBAudioDetectiveCorpusRef inCorpus, UInt64 inFirst, UInt64 inCount, UInt64* outIds /* host */);
UInt32 LBAudioDetectiveCorpusHasEntryIds(LBAudioDetectiveCorpusRef inCorpus);
OSStatus LBAudioDetectiveCorpusIdsFromKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inKeys /* device */, UInt64 inCount,
                                                 UInt64 inIndexBase, void* outIds /* device */, void* inStream);
OSStatus LBAudioDetectiveCorpusKeysFromIdsDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inIds /* device */, UInt64 inCount,
                                                 UInt64 inIndexBase, void* outKeys /* device */, void* inStream);
/* Groups: the step between a join's duplicate pairs and the removal -- the connected components of the match graph, computed on
 * the device where the keys lie, and the key list "every entry except the first of its group", which
 * LBAudioDetectiveCorpusRemoveKeysDevice and LBAudioDetectiveCorpusGatherKeysDevice take as it is.  (The join reports ORDERED
 * pairs, so a pair of near-copies shows up as i -> j and j -> i: removing the join's keys themselves removes every member of
 * every duplicate set, the original included.)  Neither call takes a corpus: they work on keys and labels alone.
 * The graph.  The vertices are the entries 0 .. inEntryCount - 1 of ONE index space (in practice a corpus joined with itself).
 * Every key slot p < inSlotCount that holds a valid key is an undirected edge {entry of p's row, entry of the key}.  A key is
 * read as the removal reads it: the low word is 0xFFFFFFFF - (inIndexBase + index), the score word is ignored, a zero key and
 * a key whose index lies outside [inIndexBase, inIndexBase + inEntryCount) are skipped; self-edges and repeated edges are
 * harmless.  A match in EITHER direction joins two entries (score(i -> j) >= t does not imply score(j -> i) >= t): a group is
 * a component of the undirected graph, and there is no "both directions only" mode.
 * The row of a slot.  inOffsets given: the join's CSR, inRowCount + 1 UInt64; slot p belongs to the last row r with
 * offsets[r] <= p, and only slots below min(offsets[inRowCount], inSlotCount) are read -- a cut list is used as far as it goes
 * and no status says so (the caller has the true total in the offsets); inRowPitch is ignored.  inOffsets NULL: pitched rows,
 * the threshold batch calls' layout; slot p belongs to row p / inRowPitch, inRowPitch >= 1 and inSlotCount == inRowCount x
 * inRowPitch, and the zero padding inside the rows is skipped.
 * The entry of a row.  inRowKeys NULL: row r is entry inFirstRow + r (the join's inFirstQuery).  inRowKeys given: inRowCount
 * keys, row r is the entry key r names and a zero or out-of-range row key makes the whole row empty (inFirstRow is ignored) --
 * the key list a LBAudioDetectiveCorpusGatherKeysDevice call was given, which serves a ragged corpus' route: gather the entries
 * of one length, query them with LBAudioDetectiveCorpusQueryPackedThresholdKeysDevice, group the key block.
 * The result.  ioLabels[i] (UInt32) is the LOWEST entry index of i's component: that entry is the group's first entry, and its
 * label is its own index.  outGroupCount, when given, receives the number of components as one UInt64.  The result is a
 * function of the edge set alone: it does not depend on launch order, grid, slot order or chunking.
 * Several calls.  inReset != 0 starts from "every entry alone"; inReset == 0 adds this call's edges to the grouping ioLabels
 * holds, so a self-join made in row chunks is grouped chunk by chunk, in any order of the chunks, into the labels of one call
 * over all edges.  Without a reset ioLabels is read as a forest -- a word below its own index is the entry's parent, any other
 * word makes the entry a group's first -- so no content of it can make the call read out of range or run on.
 * The call is asynchronous on inStream, which is never awaited; nothing is read back, the number of launches (at most three and
 * one 8-byte memset) does not depend on the data, and there is no scratch beyond the caller's buffers.
 * Decided before anything touches the device, each kLBAudioDetectiveArgumentInvalid: a NULL ioLabels; a NULL inKeys with
 * inSlotCount != 0; inIndexBase > 2^32 or inIndexBase + inEntryCount > 2^32; inSlotCount > 2^31; inRowCount > 2^32; inRowKeys
 * NULL and inFirstRow + inRowCount > inEntryCount; the pitch rules; a pointer not aligned to its element (8 bytes for keys,
 * offsets, row keys and the group count, 4 for labels).  Then a missing device is kLBAudioDetectiveDeviceUnavailable.
 * inEntryCount == 0 is noErr and writes a group count of 0; inRowCount == 0 or inSlotCount == 0 adds no edge (with inReset
 * the labels are the identity).
 * LBAudioDetectiveGroupExtraKeysFromLabelsDevice writes the key of every entry whose label is not its own index -- every entry
 * that is not its group's first -- in ascending index to the slots 0 .. min(count, inCapacity) - 1 of outKeys, zero keys
 * behind them, and the TRUE number, inEntryCount - groups, to *outCount (host).  A key's score word is the bits of 1.0f, so a
 * key is never zero, also for index 0xFFFFFFFF.  Like LBAudioDetectiveThresholdKeysFromScoresDevice the call owns its scratch
 * (8 x (ceil(inEntryCount / 1024) + 1) bytes) and returns once the keys are written.  NULL inLabels, outKeys or outCount,
 * inCapacity outside 1 .. 2^31, the index-base rules above and misaligned device pointers are
 * kLBAudioDetectiveArgumentInvalid; then a missing device is kLBAudioDetectiveDeviceUnavailable. */
OSStatus LBAudioDetectiveGroupLabelsFromKeysDevice(const void* inKeys /* device */, UInt64 inSlotCount,
                                                   const void* inOffsets /* device, inRowCount + 1 UInt64, or NULL */,
                                                   UInt64 inRowPitch, UInt64 inRowCount, UInt64 inFirstRow,
                                                   const void* inRowKeys /* device, inRowCount keys, or NULL */, UInt64 inIndexBase,
                                                   UInt64 inEntryCount, UInt32 inReset, void* ioLabels /* device, inEntryCount UInt32 */,
                                                   void* outGroupCount /* device, one UInt64, may be NULL */, void* inStream);
OSStatus LBAudioDetectiveGroupExtraKeysFromLabelsDevice(const void* inLabels /* device */, UInt64 inEntryCount, UInt64 inIndexBase,
                                                        UInt64 inCapacity, void* outKeys /* device, inCapacity keys */,
                                                        UInt64* outCount /* host */, void* inStream);
/* Where a match lies.  LBAudioDetectiveFingerprintCompareToFingerprint (Fp.m:119-149) slides the shorter fingerprint along
 * the longer one; the corpus passes the query as its first argument.  Entry longer than the query ("A"): the query slides
 * along the entry.  Otherwise ("B", equal lengths included): the entry slides along the query.  With n1 >= n2 the two counts,
 * offset o = 0 .. n1 - n2 scores q_o = (float32 sum over i = 0 .. n2 - 1, in that order, of the sub-fingerprint ratio of
 * the longer side's i + o against the shorter side's i) / n2, correctly rounded.  The entry's score is max(0, max q_o), bit
 * for bit what LBAudioDetectiveCorpusScoresDevice returns for it, and its offset the LOWEST o that reaches it.  The LAG is
 * signed: +offset in A (the query's sub-fingerprint 0 lines up with the entry's sub-fingerprint lag), -offset in B (the
 * entry's sub-fingerprint 0 lines up with the query's sub-fingerprint -lag); 0 for equal lengths.  Unused result slots
 * (index -1, a zero key) get lag 0.  One sub-fingerprint is one frame of 128 analysis windows, so for the PCM entry points
 * lag x 128 x analysis stride / processing sample rate is the position in seconds (5512 Hz, stride 64: 1.486 s per
 * sub-fingerprint); the file entry points advance by their own hop (LBAudioDetectiveSetFileHopMode) instead of the stride.
 *
 * Alignment runs after selection, on the (query, entry) pairs the top-1 / top-K paths produce; the scans are the same.
 * Arguments are checked as for the top-K calls: queries of the corpus' sub-fingerprint length, inCount >= 1,
 * 1 <= inK <= LBAD_TOPK_MAX, inIndexBase + entries <= 2^32; NULL handles and pointers are kLBAudioDetectiveArgumentInvalid,
 * and without a device every call returns kLBAudioDetectiveDeviceUnavailable.  The corpus owns the scratch, grown on demand;
 * a call waits for the previous alignment's device work before it reuses it.
 *
 * AlignKeysDevice: inCount x inK keys at the device pointer inKeys (rows as QueryBatchTopKKeysDevice writes them, query q's
 * row at q * inK, index = inIndexBase + entry) -> inCount x inK SInt32 lags at the device pointer outLags and, unless outScores
 * is NULL, the recomputed Float32 scores (equal to the keys' scores, bit for bit).  A key that is zero or names an index
 * outside [inIndexBase, inIndexBase + entries) gets lag 0 and score 0.  Asynchronous on inStream, no host round trip: the
 * building block of a sharded top-K, where every rank aligns its own keys before the merge.
 * QueryBatchTopKAligned: LBAudioDetectiveCorpusQueryBatchTopK's indices, scores and counts, bit for bit, plus the lags.
 * QueryAligned: LBAudioDetectiveCorpusQuery's index and score (bound pruning on or off) plus the winner's lag.
 * MatchProfile: every q_o of the query against entry inEntry, in offset order, to the host array outScores; *outCount =
 * n1 - n2 + 1.  Slot o's lag is *outFirstLag + o in A and *outFirstLag - o in B (*outFirstLag is 0), and the profile's maximum
 * is the entry's score.  A capacity below the count returns kLBAudioDetectiveArgumentInvalid with *outCount set (outScores may
 * then be NULL): the caller sizes the buffer and calls again. */
OSStatus LBAudioDetectiveCorpusAlignKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const LBAudioDetectiveFingerprintRef* inQueries,
                                               UInt32 inCount, UInt32 inRange, UInt32 inK, const void* inKeys, UInt64 inIndexBase,
                                               void* outLags, void* outScores, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryBatchTopKAligned(LBAudioDetectiveCorpusRef inCorpus,
                                                     const LBAudioDetectiveFingerprintRef* inQueries, UInt32 inCount,
                                                     UInt32 inRange, UInt32 inK, SInt64* outIndices, Float32* outScores,
                                                     SInt32* outLags, UInt32* outCounts);
OSStatus LBAudioDetectiveCorpusQueryAligned(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                            UInt32 inRange, SInt64* outIndex, Float32* outScore, SInt32* outLag);
OSStatus LBAudioDetectiveCorpusMatchProfile(LBAudioDetectiveCorpusRef inCorpus, LBAudioDetectiveFingerprintRef inQuery,
                                            UInt32 inRange, UInt64 inEntry, Float32* outScores, UInt64 inCapacity,
                                            UInt64* outCount, SInt32* outFirstLag);
/* Packed queries: fingerprints that are ALREADY on the device in the packed layout -- what LBAudioDetectiveFingerprintClipsDevice
 * writes and LBAudioDetectiveCorpusAppendPackedDevice reads -- queried without a handle and without a visit to the host.
 * inPackedQueries is a device pointer to inCount x inSubfingerprintsPerQuery x LBAD_PACKED_BYTES bytes: query q's
 * sub-fingerprints one after the other from byte q * inSubfingerprintsPerQuery * LBAD_PACKED_BYTES on, 4-byte alignment
 * suffices; every query of a call has the same number of sub-fingerprints (several lengths: several calls), and the
 * sub-fingerprint length is the corpus'.  Bits at or above that length are ignored.  Builder kernels turn the rows into the
 * blocks the scans read -- bit for bit what the handle-taking calls stage from a fingerprint with the same Booleans -- and the
 * same scan, selection and alignment kernels run on them, so for both corpus kinds, any inRange (0: the sub-fingerprint
 * length) and bound pruning on or off:
 * QueryPackedKeysDevice writes inCount 64-bit keys to the device pointer outKeys, equal to LBAudioDetectiveCorpusQueryBatchKeysDevice's;
 * QueryPackedTopKKeysDevice writes inCount x inK keys, equal to LBAudioDetectiveCorpusQueryBatchTopKKeysDevice's, and -- unless
 * outLags is NULL -- inCount x inK SInt32 lags to the device pointer outLags, equal to LBAudioDetectiveCorpusAlignKeysDevice's
 * on those keys.
 * Both are asynchronous on inStream; nothing of the queries is copied to the host and the stream is never awaited.  Uniform
 * corpus: the specialised shape (200 Booleans, as many sub-fingerprints as an entry, at most 8) takes the batch scan, eight
 * queries per pass, even for one query; other shapes one generic scan per query, whose query must fit 48 KiB.  Ragged corpus:
 * the queries share launches as in LBAudioDetectiveCorpusQueryBatchKeysDevice.  LBAudioDetectiveCorpusSetKernelVariant means what
 * it means for the handle-taking calls (2 on a shape without the specialised scan: kLBAudioDetectiveArgumentInvalid).
 * kLBAudioDetectiveArgumentInvalid: a NULL corpus or pointer (outLags excepted), inCount == 0, inSubfingerprintsPerQuery == 0,
 * inK outside 1 .. LBAD_TOPK_MAX, inIndexBase + entries > 2^32, inCount x inSubfingerprintsPerQuery > 2^32 - 1, with lags
 * inSubfingerprintsPerQuery > 0x7FFFFFFF; without a device kLBAudioDetectiveDeviceUnavailable.  An empty corpus gives zero keys
 * and zero lags.  The corpus owns the builders' output, grown on demand; a call waits for the previous packed call's device
 * work before it reuses it (and, as the calls it mirrors, for the previous top-K call and alignment). */
OSStatus LBAudioDetectiveCorpusQueryPackedKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                     UInt32 inCount, UInt32 inSubfingerprintsPerQuery, UInt32 inRange,
                                                     UInt64 inIndexBase, void* outKeys, void* inStream);
OSStatus LBAudioDetectiveCorpusQueryPackedTopKKeysDevice(LBAudioDetectiveCorpusRef inCorpus, const void* inPackedQueries,
                                                         UInt32 inCount, UInt32 inSubfingerprintsPerQuery, UInt32 inRange,
                                                         UInt32 inK, UInt64 inIndexBase, void* outKeys, void* outLags,
                                                         void* inStream);
/* Debug / tests: the query blocks themselves, copied to the host array outWords (*outCount words; a capacity below that, or a
 * NULL outWords, returns kLBAudioDetectiveArgumentInvalid with *outCount set).  Exactly one source: inPackedQueries (device,
 * as above; the builder kernels run on the null stream) or inBooleans (host, inCount x inPer x inSubfingerprintLength
 * Booleans; the builders behind the handle-taking calls, no device needed).  inKind 0: the specialised uniform scan's blocks
 * (length 200, inPer <= 8 sub-fingerprints per query and entry; 144 words per query); 1: the ragged scan's blocks
 * ((inPer + 1) x 16 words); 2 / 3: the alignment's words for a ragged / uniform corpus (inPer x 8 words; 3 is also the generic
 * uniform scan's query). */
OSStatus LBAudioDetectiveDebugQueryBlocks(UInt32 inKind, const void* inPackedQueries, const Boolean* inBooleans, UInt32 inCount,
                                          UInt32 inPer, UInt32 inSubfingerprintLength, UInt32 inRange, UInt32* outWords,
                                          UInt64 inCapacity, UInt64* outCount);
/* Debug / tests: which kernel ONE launch of a ragged-corpus scan takes and what it needs in front of it -- the scan's own
 * decision (sliding.cpp: sliding_choose) as words; touches no device.  The corpus is described by a histogram of entry lengths
 * (inLengthCount pairs of length and count), its record count, its longest entry and its kernel variant; the launch by the
 * query length, the queries of that length still to go, the range (0: the whole length), whether per-entry scores are wanted,
 * whether the query blocks are on the host, and the device's compute units.  outWords (inCapacity >= 21):
 *   0 queries this launch takes (0: no such launch, every other word is 0)   1 family: 0 compare_sliding_kernel, 1
 *   compare_short_kernel, 2 compare_short_multi_kernel   2..5 the instance's template arguments (FULL, QLDS, QN, THREADS | K, QN |
 *   QN, NQ)   6 b_min   7..8 tasks_a   9..10 tasks_b (low, high)   11..13 grid, chunk_a, chunk_b   14 the plan is read   15 the
 *   query travels in the kernel's arguments   16 the launch maxes its keys in place   17 a systolic launch follows, with 18 its
 *   look and 19 its only_upto   20 look of a systolic first launch */
OSStatus LBAudioDetectiveDebugSlidingChoice(const UInt32* inEntryLengths, const UInt64* inEntryCounts, UInt32 inLengthCount,
                                            UInt64 inRecordCount, UInt32 inLongestEntry, UInt32 inKernelVariant,
                                            UInt32 inSubfingerprintLength, UInt32 inQueryLength, UInt32 inQueriesLeft, UInt32 inRange,
                                            UInt32 inScores, UInt32 inHostBlocks, UInt32 inComputeUnits, UInt32* outWords,
                                            UInt32 inCapacity);
/* Debug / tests: bytes of device and of pinned host memory that detectives and corpora of this process hold right now, scratch of
 * single calls included.  The process-wide contexts of the pair compare, the Frame API and the sharded query, and what
 * LBAudioDetectiveDeviceMalloc hands out, are not counted.  Needs no device. */
OSStatus LBAudioDetectiveDebugLiveBytes(UInt64* outDevice, UInt64* outPinned);
/* Debug / TESTS ONLY: a process-wide ceiling on the workgroups of every launch whose workgroups walk work items beyond their
 * grid with a stride and carry state in LDS from one item to the next -- the occurrences, recording and timeline passes, both
 * joins and their row scan, the alignment's three launches and the threshold list's count and scatter -- and of the plain
 * grid-stride launches of the stream bank, the resampler bank, the duplicate groups (init, hook, flatten), the gather's two
 * copy launches, the top-K selection's histogram and gather passes (grid.x; the rows stay in grid.y) and all six launches of the
 * entry ids (ids from keys, the index's init and insert, keys from ids, the removal's id gather and scatter).  Each of them launches
 * min(its work, its built-in ceiling, inWorkgroups) workgroups, never fewer than 1; 0 (the default) restores the built-in
 * ceilings alone.  Results NEVER depend on the value: it only decides how many work items one workgroup takes, which is how a
 * test of seconds reaches the trips that otherwise need a corpus of a million entries.  The second call reports the ceiling
 * and how many launches of this process so far had a grid below their work (it never decreases); it fails with
 * kLBAudioDetectiveArgumentInvalid when a pointer is NULL.  Neither needs a device. */
OSStatus LBAudioDetectiveDebugSetGridCeiling(UInt32 inWorkgroups);
OSStatus LBAudioDetectiveDebugGridCeiling(UInt32* outWorkgroups, UInt64* outStridedLaunches);
/* Binary corpus file ("LBADCRP1" header + the stored entries' planes; a ragged corpus: "LBADCRP2" header + the
 * entries' sub-fingerprint counts + the records); Load recognises both, reserves max(inCapacity, stored count)
 * entries and, for a ragged corpus, records in proportion.  A corpus with entry ids writes the "LBADIDS1" trailer behind either
 * payload (see Entry ids); one without writes exactly the bytes above. */
OSStatus LBAudioDetectiveCorpusSave(LBAudioDetectiveCorpusRef inCorpus, const char* inPath);
LBAudioDetectiveCorpusRef LBAudioDetectiveCorpusLoad(const char* inPath, UInt64 inCapacity);
/* Kernel selection: 0 = automatic, 1 = generic kernel, 2 = specialised plane kernel.  Ragged corpora only: 3 = always hand
 * the entries of fewer than 16 sub-fingerprints that are not longer than the query to the systolic scan (a second launch;
 * automatic: when their share of the work makes it pay), 4 = never. */
OSStatus LBAudioDetectiveCorpusSetKernelVariant(LBAudioDetectiveCorpusRef inCorpus, UInt32 inVariant);

/* ---- synthetic inputs generated on the device (bench / tests) -------------------------- */
/* Integer-arithmetic generator; bit-identical to oracle/lbad_oracle.c:lbo_synth_clip. */
OSStatus LBAudioDetectiveSynthClipsDevice(UInt32 inSeed, UInt64 inFirstClip, UInt64 inNumberOfClips,
                                          UInt32 inSampleRateHz, UInt32 inSamplesPerClip, UInt32 inStereoSum,
                                          Float32* outClips, void* inStream);
/* Ragged form: entry e = sub-fingerprints [inOffsets[e], inOffsets[e + 1]) of the output (inOffsets: DEVICE
 * array of inNumberOfEntries + 1 uint32, inOffsets[0] = 0); sub-fingerprint s of entry e is lbo_synth_entry's. */
OSStatus LBAudioDetectiveSynthRaggedCorpusDevice(UInt32 inSeed, UInt64 inFirstEntry, UInt64 inNumberOfEntries,
                                                 const UInt32* inOffsets, UInt64 inTotalSubfingerprints,
                                                 UInt32 inSubfingerprintLength, void* outPacked, void* inStream);
/* Packed batch layout (entries x perEntry x LBAD_PACKED_BYTES); matches lbo_synth_entry. */
OSStatus LBAudioDetectiveSynthCorpusDevice(UInt32 inSeed, UInt64 inFirstEntry, UInt64 inNumberOfEntries,
                                           UInt32 inSubfingerprintsPerEntry, UInt32 inSubfingerprintLength,
                                           void* outPacked, void* inStream);

/* ---- minimal device plumbing for hosts without a HIP binding --------------------------- */
SInt32 LBAudioDetectiveDeviceCount(void);
OSStatus LBAudioDetectiveDeviceSet(SInt32 inDevice);   /* the current device of this thread (one process drives one GPU) */
OSStatus LBAudioDetectiveDeviceMalloc(void** outPointer, UInt64 inBytes);
OSStatus LBAudioDetectiveDeviceFree(void* inPointer);
OSStatus LBAudioDetectiveDeviceCopyIn(void* inDevice, const void* inHost, UInt64 inBytes);
OSStatus LBAudioDetectiveDeviceCopyOut(void* inHost, const void* inDevice, UInt64 inBytes);
OSStatus LBAudioDetectiveDeviceSynchronize(void);
/* Measurement aid: shader clock (MHz) averaged over inMicroseconds, read inside a one-wave kernel on inStream
 * (s_memtime against the constant 100 MHz s_memrealtime) -- launched on a side stream it reports the clock the
 * chip runs at UNDER the load of whatever else is executing.  Synchronises inStream. */
OSStatus LBAudioDetectiveProbeShaderClock(void* inStream, UInt32 inMicroseconds, Float64* outMegahertz);
const char* LBAudioDetectiveVersionString(void);

#ifdef __cplusplus
}
#endif

#ifdef __OBJC__
/* Objective-C hosts: upstream's NSURL-taking names (D.h:218,235), source compatible with
 * LBAudioDetectiveTests.m:66-68 and the README snippet.  The path is taken with two message sends through the
 * runtime's objc_msgSend; under ARC the intermediate NSString lives until the call has returned. */
#if defined(__has_include)
#if __has_include(<objc/message.h>)
#include <objc/message.h>
#define LBAD_HAVE_OBJC_MESSAGE_H 1
#endif
#endif
#ifndef LBAD_HAVE_OBJC_MESSAGE_H
#ifdef __cplusplus
extern "C" id objc_msgSend(id, SEL, ...);
#else
extern id objc_msgSend(id, SEL, ...);
#endif
#endif
static inline const char* LBAudioDetectivePathOfURL(NSURL* inURL) {
    id path;
    if (!inURL) return (const char*)0;
    path = ((id (*)(id, SEL))(void (*)(void))objc_msgSend)((id)inURL, @selector(path));
    return path ? ((const char* (*)(id, SEL))(void (*)(void))objc_msgSend)(path, @selector(fileSystemRepresentation)) : (const char*)0;
}
static inline OSStatus LBAudioDetectiveProcessAudioURL(LBAudioDetectiveRef inDetective, NSURL* inFileURL,
                                                       LBAudioDetectiveFingerprintRef* outFingerprint) {   /* D.h:218 */
    return LBAudioDetectiveProcessAudioPath(inDetective, LBAudioDetectivePathOfURL(inFileURL), outFingerprint);
}
static inline OSStatus LBAudioDetectiveCompareAudioURLs(LBAudioDetectiveRef inDetective, NSURL* inFileURL1, NSURL* inFileURL2,
                                                        UInt32 inComparisonRange, Float32* outMatch) {   /* D.h:235 */
    return LBAudioDetectiveCompareAudioPaths(inDetective, LBAudioDetectivePathOfURL(inFileURL1),
                                             LBAudioDetectivePathOfURL(inFileURL2), inComparisonRange, outMatch);
}
#endif /* __OBJC__ */
#endif /* LBAUDIODETECTIVE_H */
