"""MI355X-native LBAudioDetective hot path: HIP kernels behind the reference's C interface.

`lbaudiodetective_amd._native.lib()` loads lib/liblbaudiodetective.so (built by
`_native.build()` / `__graft_entry__.build()`); there is no CPU or PyTorch fallback.
"""
from ._native import build, lib, constant, LIB_PATH, PACKED_BYTES, PACKED_WORDS, ROWS_PER_FRAME, SHARD_KEYS  # noqa: F401
from .api import (  # noqa: F401
    Comm, Corpus, Detective, Fingerprint, Frame, Stream, StreamBank, ResamplerBank, LBAudioDetectiveError, noErr, pack_subfingerprint,
    frames_to_subfingerprints_device, compact_layout, compact_bands, probe_shader_clock, read_audio_url, synth_clips_device, synth_corpus_device, synth_ragged_corpus_device, unpack_packed, unpack_subfingerprint,
    decode_topk_keys, topk_keys_from_scores_device, identify_clips_device, debug_query_blocks, debug_sliding_choice, debug_stage1_choice, debug_live_bytes,
    debug_set_grid_ceiling, debug_grid_ceiling, debug_stream_bank_plan, debug_resampler_bank_plan,
    decode_threshold_keys, threshold_keys_from_scores_device, decode_join_keys, decode_occurrence_keys,
    group_labels_from_keys_device, group_extra_keys_from_labels_device, decode_timeline_keys, timeline_segments,
    decode_timeline_batch_keys, debug_timeline_batch_plan, debug_set_timeline_batch_form, timeline_segments_device, decode_segments,
    debug_recording_batch_plan, debug_set_recording_batch_form, debug_occurrences_batch_plan, debug_set_occurrences_batch_form,
    debug_occurrences_tail_plan, decode_tail_occurrences, debug_recording_tail_plan, decode_tail_matches,
    debug_occurrences_tail_peaks_plan, debug_timeline_tail_plan, LiveTimeline,
    occurrence_segments, occurrence_segments_device, decode_occurrence_segments, phase_sample_offset,
)
from .sharded import (  # noqa: F401
    ShardedCorpus, broadcast_fingerprint, gather_packed, gather_topk_aligned, make_comm, merge_topk_aligned, merge_topk_keys, shard_range,
    gather_threshold_keys, merge_threshold_keys,
)

__all__ = [
    "build", "lib", "constant", "Corpus", "Detective", "Fingerprint", "Frame", "Stream", "StreamBank", "ResamplerBank", "LBAudioDetectiveError",
    "Comm", "ShardedCorpus", "broadcast_fingerprint", "make_comm", "shard_range", "read_audio_url", "frames_to_subfingerprints_device", "compact_layout", "compact_bands", "pack_subfingerprint", "unpack_subfingerprint", "unpack_packed",
    "synth_clips_device", "synth_corpus_device", "synth_ragged_corpus_device",
    "decode_topk_keys", "topk_keys_from_scores_device", "identify_clips_device", "debug_query_blocks", "debug_sliding_choice", "debug_stage1_choice", "debug_live_bytes", "merge_topk_keys", "merge_topk_aligned", "gather_topk_aligned",
    "decode_threshold_keys", "threshold_keys_from_scores_device", "merge_threshold_keys", "gather_threshold_keys",
    "decode_join_keys", "decode_occurrence_keys", "group_labels_from_keys_device", "group_extra_keys_from_labels_device",
    "decode_timeline_keys", "timeline_segments", "debug_set_grid_ceiling", "debug_grid_ceiling", "debug_stream_bank_plan",
    "debug_resampler_bank_plan", "decode_timeline_batch_keys", "debug_timeline_batch_plan", "debug_set_timeline_batch_form",
    "timeline_segments_device", "decode_segments", "debug_recording_batch_plan", "debug_set_recording_batch_form",
    "debug_occurrences_batch_plan", "debug_set_occurrences_batch_form", "debug_occurrences_tail_plan", "decode_tail_occurrences",
    "debug_recording_tail_plan", "decode_tail_matches", "debug_occurrences_tail_peaks_plan", "debug_timeline_tail_plan", "LiveTimeline",
    "occurrence_segments", "occurrence_segments_device", "decode_occurrence_segments", "phase_sample_offset",
]
