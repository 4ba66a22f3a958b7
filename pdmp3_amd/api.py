"""ctypes mirror of include/pdmp3.h (pdmp3_amd/libpdmp3.so): the reference's
libmpg123-style streaming API, names and semantics unchanged.  Used by tests
and examples; the library itself is plain C."""
import ctypes as C
import os

import numpy as np

from .hip import SIDE_DTYPE

_HERE = os.path.dirname(os.path.abspath(__file__))
PDMP3_OK, PDMP3_ERR, PDMP3_NEED_MORE, PDMP3_NEW_FORMAT, PDMP3_NO_SPACE = 0, -1, -10, -11, 7
PDMP3_ENC_SIGNED_16 = 0xD0
_LIB = None

BULK_EXPORTS = ["pdmp3_amd_bulk_new", "pdmp3_amd_bulk_new_ex", "pdmp3_amd_bulk_new_on", "pdmp3_amd_bulk_delete", "pdmp3_amd_bulk_threads", "pdmp3_amd_bulk_split_scans", "pdmp3_amd_bulk_huffman_frames", "pdmp3_amd_bulk_set_quirks",
                "pdmp3_amd_scan_buffer", "pdmp3_amd_scan_buffer_iso", "pdmp3_amd_corpus_assign", "pdmp3_amd_corpus_decode", "pdmp3_amd_bulk_decode", "pdmp3_amd_bulk_decode_async", "pdmp3_amd_bulk_wait", "pdmp3_amd_bulk_new_parse_only", "pdmp3_amd_bulk_parse",
                "pdmp3_amd_bulk_new_parse_bits", "pdmp3_amd_bulk_new_parse_bits_lsf", "pdmp3_amd_bulk_parse_bits", "pdmp3_amd_bulk_parse_pool", "pdmp3_amd_pcm_alloc", "pdmp3_amd_pcm_free", "pdmp3_amd_stream_loop", "pdmp3_amd_write_wav",
                "pdmp3_amd_index_new", "pdmp3_amd_index_new_spacing", "pdmp3_amd_index_delete", "pdmp3_amd_index_frames", "pdmp3_amd_index_pcm_offset",
                "pdmp3_amd_index_pcm_offsets", "pdmp3_amd_index_split", "pdmp3_amd_bulk_decode_clips", "pdmp3_amd_bulk_clip_stats", "pdmp3_amd_bulk_parse_range",
                "pdmp3_amd_index_format", "pdmp3_amd_index_samples", "pdmp3_amd_audio_span", "pdmp3_amd_audio_table", "pdmp3_amd_bulk_decode_clips_audio",
                "pdmp3_amd_audio_lds_plan",
                "pdmp3_amd_mel_check", "pdmp3_amd_mel_span", "pdmp3_amd_mel_dft_table", "pdmp3_amd_mel_filterbank", "pdmp3_amd_mel_tile",
                "pdmp3_amd_bulk_decode_clips_mel",
                "pdmp3_amd_fbank_check", "pdmp3_amd_fbank_dft_length", "pdmp3_amd_fbank_table", "pdmp3_amd_fbank_filterbank", "pdmp3_amd_fbank_valid",
                "pdmp3_amd_fbank_tile", "pdmp3_amd_bulk_decode_clips_fbank",
                "pdmp3_amd_mfcc_check", "pdmp3_amd_mfcc_dct_table", "pdmp3_amd_mfcc_tile", "pdmp3_amd_bulk_decode_clips_mfcc",
                "pdmp3_amd_stft_check", "pdmp3_amd_stft_table", "pdmp3_amd_stft_tile", "pdmp3_amd_bulk_decode_clips_stft",
                "pdmp3_amd_stft_long_check", "pdmp3_amd_stft_long_tables", "pdmp3_amd_stft_long_plan", "pdmp3_amd_bulk_decode_clips_stft_long",
                "pdmp3_amd_mel_long_check", "pdmp3_amd_mel_long_filterbank", "pdmp3_amd_mel_long_operand", "pdmp3_amd_mel_long_plan",
                "pdmp3_amd_bulk_decode_clips_mel_long",
                "pdmp3_amd_cqt_check", "pdmp3_amd_cqt_lengths", "pdmp3_amd_cqt_table", "pdmp3_amd_cqt_plan", "pdmp3_amd_bulk_decode_clips_cqt",
                "pdmp3_amd_chroma_check", "pdmp3_amd_chroma_map", "pdmp3_amd_chroma_plan", "pdmp3_amd_bulk_decode_clips_chroma",
                "pdmp3_amd_loudness_check", "pdmp3_amd_loudness_coefficients", "pdmp3_amd_loudness_tables", "pdmp3_amd_loudness_plan",
                "pdmp3_amd_bulk_decode_clips_loudness",
                "pdmp3_amd_r128_check", "pdmp3_amd_r128_taps", "pdmp3_amd_r128_plan", "pdmp3_amd_bulk_decode_clips_r128",
                "pdmp3_amd_pitch_check", "pdmp3_amd_pitch_lags", "pdmp3_amd_pitch_plan", "pdmp3_amd_bulk_decode_clips_pitch",
                "pdmp3_amd_tempogram_check", "pdmp3_amd_tempogram_window", "pdmp3_amd_tempogram_prior", "pdmp3_amd_tempogram_plan",
                "pdmp3_amd_bulk_decode_clips_tempogram",
                "pdmp3_amd_spectral_check", "pdmp3_amd_spectral_plan", "pdmp3_amd_bulk_decode_clips_spectral",
                "pdmp3_amd_hpss_check", "pdmp3_amd_hpss_plan", "pdmp3_amd_bulk_decode_clips_hpss",
                "pdmp3_amd_mfcc_long_check", "pdmp3_amd_mfcc_long_dct_table", "pdmp3_amd_mfcc_long_delta_taps", "pdmp3_amd_mfcc_long_plan",
                "pdmp3_amd_bulk_decode_clips_mfcc_long",
                "pdmp3_amd_pyin_check", "pdmp3_amd_pyin_tables", "pdmp3_amd_pyin_plan", "pdmp3_amd_bulk_decode_clips_pyin",
                "pdmp3_amd_beat_check", "pdmp3_amd_beat_tables", "pdmp3_amd_beat_plan", "pdmp3_amd_bulk_decode_clips_beats"]

# include/pdmp3_hip.h: pdmp3_gc_bits / pdmp3_frame_bits
GC_BITS_DTYPE = np.dtype([("part2_3_length", "<u2"), ("big_values", "<u2"), ("global_gain", "u1"), ("scalefac_compress", "u1"),
                          ("flags", "u1"), ("table_select", "u1", (3,)), ("subblock_gain", "u1", (3,)),
                          ("region0_count", "u1"), ("region1_count", "u1"), ("count1table_select", "u1")])
FRAME_BITS_DTYPE = np.dtype([("frame", "u1"), ("scfsi", "u1", (2,)), ("iso", "u1"), ("lsf", "u1"), ("sfc_hi", "u1"), ("reserved", "u1", (10,)), ("gc", GC_BITS_DTYPE, (4,))])
RESERVOIR_BYTES = 2064
API_EXPORTS = ["pdmp3_new", "pdmp3_delete", "pdmp3_open_feed", "pdmp3_feed", "pdmp3_read",
               "pdmp3_decode", "pdmp3_getformat", "pdmp3", "pdmp3_amd_set_encoding", "pdmp3_amd_set_quirks"]
# include/pdmp3.h: the ISO-correct switches
ISO_TABLE33, ISO_MS_BOUND, ISO_IS_SHORT, ISO_SF21, ISO_SF12, ISO_IS_BOUND, ISO_ALL = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x3f
ISO_LSF = 0x40            # include/pdmp3.h PDMP3_ISO_LSF: MPEG-2 LSF / MPEG-2.5 streams are decoded (the reference rejects them)
PDMP3_ENC_SIGNED_16, PDMP3_ENC_FLOAT_32 = 0xD0, 0x200


def library_path():
    # PDMP3_HOST_LIB: alternative build of the host library (A/B experiments; it brings the engine library it was linked with)
    return os.environ.get("PDMP3_HOST_LIB") or os.path.join(_HERE, "libpdmp3.so")


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError("pdmp3_amd: %s is missing -- run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    vp = C.c_void_p
    lib.pdmp3_new.restype = vp
    lib.pdmp3_new.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
    lib.pdmp3_delete.argtypes = [vp]
    lib.pdmp3_open_feed.argtypes = [vp]
    lib.pdmp3_feed.argtypes = [vp, vp, C.c_size_t]
    lib.pdmp3_read.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.pdmp3_decode.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.pdmp3_getformat.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.pdmp3_amd_set_encoding.argtypes = [vp, C.c_int]
    lib.pdmp3_amd_new_parse_only.restype = vp
    lib.pdmp3_amd_set_tap.argtypes = [vp, vp, vp, C.c_int]
    lib.pdmp3_amd_tap_count.argtypes = [vp]
    lib.pdmp3_amd_parse_available.argtypes = [vp]
    # include/pdmp3_bulk.h
    lib.pdmp3_amd_bulk_new.restype = vp
    lib.pdmp3_amd_bulk_new.argtypes = [C.c_int, C.c_int]
    lib.pdmp3_amd_bulk_new_parse_only.restype = vp
    lib.pdmp3_amd_bulk_new_parse_only.argtypes = [C.c_int, C.c_int]
    lib.pdmp3_amd_bulk_delete.argtypes = [vp]
    lib.pdmp3_amd_bulk_threads.argtypes = [vp]
    if hasattr(lib, "pdmp3_amd_bulk_split_scans"):          # (absent from builds before round 5's end: PDMP3_HOST_LIB A/B runs)
        lib.pdmp3_amd_bulk_split_scans.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        lib.pdmp3_amd_bulk_split_scans.restype = None
    lib.pdmp3_amd_scan_buffer.restype = C.c_longlong
    lib.pdmp3_amd_scan_buffer.argtypes = [vp, C.c_size_t, C.POINTER(C.c_longlong)]
    lib.pdmp3_amd_bulk_decode.restype = C.c_longlong
    lib.pdmp3_amd_bulk_decode.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_int)]
    lib.pdmp3_amd_bulk_new_ex.restype = vp
    lib.pdmp3_amd_bulk_new_ex.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.pdmp3_amd_bulk_new_on.restype = vp
    lib.pdmp3_amd_bulk_new_on.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    lib.pdmp3_amd_bulk_new_parse_bits.restype = vp
    lib.pdmp3_amd_bulk_new_parse_bits.argtypes = []
    lib.pdmp3_amd_bulk_new_parse_bits_lsf.restype = vp
    lib.pdmp3_amd_bulk_new_parse_bits_lsf.argtypes = []
    lib.pdmp3_amd_bulk_huffman_frames.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.pdmp3_amd_bulk_huffman_frames.restype = None
    lib.pdmp3_amd_bulk_parse_bits.restype = C.c_longlong
    lib.pdmp3_amd_bulk_parse_bits.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_longlong)]
    lib.pdmp3_amd_bulk_decode_async.restype = C.c_longlong
    lib.pdmp3_amd_bulk_decode_async.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_int)]
    lib.pdmp3_amd_bulk_wait.argtypes = [vp]
    lib.pdmp3_amd_pcm_alloc.restype = vp
    lib.pdmp3_amd_pcm_alloc.argtypes = [C.c_size_t]
    lib.pdmp3_amd_pcm_free.argtypes = [vp]
    lib.pdmp3_amd_bulk_parse.restype = C.c_longlong
    lib.pdmp3_amd_bulk_parse.argtypes = [vp, vp, C.c_size_t, vp, vp, C.c_size_t, C.POINTER(C.c_longlong)]
    if hasattr(lib, "pdmp3_amd_index_new_spacing"):          # (frame ranges and clips: absent from older builds, PDMP3_HOST_LIB A/B runs)
        ll = C.c_longlong
        lib.pdmp3_amd_index_new_spacing.restype = vp
        lib.pdmp3_amd_index_new_spacing.argtypes = [vp, C.c_size_t, C.c_uint, C.c_int]
        lib.pdmp3_amd_index_delete.argtypes = [vp]
        lib.pdmp3_amd_index_delete.restype = None
        lib.pdmp3_amd_index_frames.argtypes = [vp]
        lib.pdmp3_amd_index_frames.restype = ll
        lib.pdmp3_amd_index_pcm_offsets.argtypes = [vp, vp, C.c_size_t]
        lib.pdmp3_amd_index_pcm_offsets.restype = ll
        lib.pdmp3_amd_index_split.argtypes = [vp]
        lib.pdmp3_amd_bulk_decode_clips.argtypes = [vp, vp, C.c_int, vp]
        lib.pdmp3_amd_bulk_clip_stats.argtypes = [vp, C.POINTER(ll), C.POINTER(ll)]
        lib.pdmp3_amd_bulk_clip_stats.restype = None
        lib.pdmp3_amd_bulk_parse_range.argtypes = [vp, vp, C.c_size_t, vp, ll, ll, C.c_int, vp, vp, C.c_size_t, C.POINTER(ll)]
        lib.pdmp3_amd_bulk_parse_range.restype = ll
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_audio"):    # (clips as float batches: absent from older builds)
        ll = C.c_longlong
        lib.pdmp3_amd_index_format.argtypes = [vp, C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_index_samples.argtypes = [vp]
        lib.pdmp3_amd_index_samples.restype = ll
        lib.pdmp3_amd_audio_span.argtypes = [C.c_long, C.c_long, C.c_int, C.c_double, ll, ll, C.POINTER(ll), C.POINTER(ll)]
        lib.pdmp3_amd_audio_table.argtypes = [C.c_long, C.c_long, C.c_int, C.c_double, vp, C.c_size_t, C.POINTER(C.c_long), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_audio_table.restype = ll
        lib.pdmp3_amd_bulk_decode_clips_audio.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_audio_lds_plan"):             # (the LDS plan of a pair, for the tests: absent from older builds)
        lib.pdmp3_amd_audio_lds_plan.argtypes = [C.c_long, C.c_long, C.c_int, C.c_double, C.c_int, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_mel"):      # (log-mel features of clips: absent from older builds)
        lib.pdmp3_amd_mel_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_mel_span.argtypes = [C.c_int, C.c_int, ll, ll, C.POINTER(ll), C.POINTER(ll)]
        lib.pdmp3_amd_mel_dft_table.argtypes = [C.c_int, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_mel_dft_table.restype = ll
        lib.pdmp3_amd_mel_filterbank.argtypes = [C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t]
        lib.pdmp3_amd_mel_filterbank.restype = ll
        lib.pdmp3_amd_mel_tile.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_mel.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_fbank"):    # (Kaldi-style filterbank features of clips: absent from older builds)
        lib.pdmp3_amd_fbank_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_fbank_dft_length.argtypes = [C.c_int, C.c_int]
        lib.pdmp3_amd_fbank_table.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_fbank_table.restype = ll
        lib.pdmp3_amd_fbank_filterbank.argtypes = [C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, vp, C.c_size_t]
        lib.pdmp3_amd_fbank_filterbank.restype = ll
        lib.pdmp3_amd_fbank_valid.argtypes = [ll, ll, C.c_int, C.c_int, ll]
        lib.pdmp3_amd_fbank_valid.restype = ll
        lib.pdmp3_amd_fbank_tile.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_fbank.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_mfcc"):     # (Kaldi-style MFCC features of clips: absent from older builds)
        lib.pdmp3_amd_mfcc_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_mfcc_dct_table.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_mfcc_dct_table.restype = ll
        lib.pdmp3_amd_mfcc_tile.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_mfcc.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_stft"):     # (the short-time Fourier transform of clips: absent from older builds)
        lib.pdmp3_amd_stft_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_stft_table.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_stft_table.restype = ll
        lib.pdmp3_amd_stft_tile.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_stft.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_stft_long"):    # (... at n_fft 2048 and 4096: absent from older builds)
        lib.pdmp3_amd_stft_long_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_stft_long_tables.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_int)]
        lib.pdmp3_amd_stft_long_tables.restype = ll
        lib.pdmp3_amd_stft_long_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_stft_long.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_mel_long"):     # (log-mel features at n_fft 2048 and 4096: absent from older builds)
        lib.pdmp3_amd_mel_long_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_mel_long_filterbank.argtypes = [C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t]
        lib.pdmp3_amd_mel_long_filterbank.restype = ll
        lib.pdmp3_amd_mel_long_operand.argtypes = [C.c_long, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.c_size_t,
                                                   C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_mel_long_operand.restype = ll
        lib.pdmp3_amd_mel_long_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_mel_long.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_cqt"):          # (the constant-Q transform of clips: absent from older builds)
        lib.pdmp3_amd_cqt_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_cqt_lengths.argtypes = [vp, C.c_long, vp, vp, C.c_size_t]
        lib.pdmp3_amd_cqt_table.argtypes = [vp, C.c_long, vp, C.c_size_t, vp, vp]
        lib.pdmp3_amd_cqt_table.restype = ll
        lib.pdmp3_amd_cqt_plan.argtypes = [vp, C.c_long] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_uint)] + [C.POINTER(C.c_int)] * 3
        lib.pdmp3_amd_bulk_decode_clips_cqt.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_chroma"):       # (chroma features of clips: absent from older builds)
        lib.pdmp3_amd_chroma_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_chroma_map.argtypes = [vp, C.c_long, vp, C.c_size_t, vp]
        lib.pdmp3_amd_chroma_plan.argtypes = [vp, C.c_long] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_uint)] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_uint)] * 2
        lib.pdmp3_amd_bulk_decode_clips_chroma.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_loudness"):     # (loudness of clips: absent from older builds)
        lib.pdmp3_amd_loudness_check.argtypes = [vp, C.c_long, C.c_int]
        lib.pdmp3_amd_loudness_coefficients.argtypes = [C.c_long, vp]
        lib.pdmp3_amd_loudness_tables.argtypes = [C.c_long, vp, vp, vp, vp, vp]
        lib.pdmp3_amd_loudness_plan.argtypes = [C.c_long, ll] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_uint), C.POINTER(C.c_int)] + [C.POINTER(ll)] * 3
        lib.pdmp3_amd_bulk_decode_clips_loudness.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_r128"):         # (true peak, short-term loudness, loudness range: absent from older builds)
        lib.pdmp3_amd_r128_check.argtypes = [vp, C.c_long, C.c_int]
        lib.pdmp3_amd_r128_taps.argtypes = [vp, vp]
        lib.pdmp3_amd_r128_plan.argtypes = [C.c_long, ll] + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_uint), C.POINTER(C.c_int)] + [C.POINTER(ll)] * 6
        lib.pdmp3_amd_bulk_decode_clips_r128.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_pitch"):        # (pitch of clips: absent from older builds)
        lib.pdmp3_amd_pitch_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_pitch_lags.argtypes = [vp, C.c_long] + [C.POINTER(C.c_int)] * 3
        lib.pdmp3_amd_pitch_plan.argtypes = [vp, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_int)]
        lib.pdmp3_amd_bulk_decode_clips_pitch.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_pyin"):         # (pYIN pitch tracking: absent from older builds)
        lib.pdmp3_amd_pyin_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_pyin_tables.argtypes = [vp, C.c_long, vp, C.c_size_t, C.POINTER(C.c_int)]
        lib.pdmp3_amd_pyin_plan.argtypes = [vp, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)]
        lib.pdmp3_amd_bulk_decode_clips_pyin.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_beats"):        # (beat tracking: absent from older builds)
        lib.pdmp3_amd_beat_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_beat_tables.argtypes = [vp, C.c_long, C.c_int, vp, vp]
        lib.pdmp3_amd_beat_plan.argtypes = [vp, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)]
        lib.pdmp3_amd_bulk_decode_clips_beats.argtypes = [vp, vp, C.c_int, vp, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_tempogram"):    # (onset strength, tempogram, tempo: absent from older builds)
        lib.pdmp3_amd_tempogram_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_tempogram_window.argtypes = [C.c_int, vp, C.c_size_t]
        lib.pdmp3_amd_tempogram_prior.argtypes = [vp, C.c_long, vp, C.c_size_t, C.POINTER(C.c_int)]
        lib.pdmp3_amd_tempogram_plan.argtypes = [vp, C.c_long] + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_tempogram.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_spectral"):     # (spectral descriptors at n_fft 2048 and 4096: absent from older builds)
        lib.pdmp3_amd_spectral_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_spectral_plan.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_spectral.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_hpss"):         # (harmonic-percussive separation: absent from older builds)
        lib.pdmp3_amd_hpss_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_hpss_plan.argtypes = [C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_hpss.argtypes = [vp, vp, C.c_int, vp, vp]
    if hasattr(lib, "pdmp3_amd_bulk_decode_clips_mfcc_long"):    # (librosa-style MFCC, deltas, dB mel: absent from older builds)
        lib.pdmp3_amd_mfcc_long_check.argtypes = [vp, C.c_long]
        lib.pdmp3_amd_mfcc_long_dct_table.argtypes = [C.c_int, C.c_int, C.c_double, vp, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        lib.pdmp3_amd_mfcc_long_dct_table.restype = ll
        lib.pdmp3_amd_mfcc_long_delta_taps.argtypes = [C.c_int, vp, C.c_size_t]
        lib.pdmp3_amd_mfcc_long_plan.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_uint)]
        lib.pdmp3_amd_bulk_decode_clips_mfcc_long.argtypes = [vp, vp, C.c_int, vp, vp]
    _LIB = lib
    return lib


class Decoder:
    """pdmp3_handle wrapper.  parse_only=True gives the GPU-less test handle."""

    def __init__(self, parse_only=False):
        self.lib = load_library()
        if parse_only:
            self.h = self.lib.pdmp3_amd_new_parse_only()
        else:
            err = C.c_int(0)
            self.h = self.lib.pdmp3_new(None, C.byref(err))
        if not self.h:
            raise RuntimeError("pdmp3_new failed (no MI355X transform engine; there is no CPU fallback)")
        self.lib.pdmp3_open_feed(self.h)

    def close(self):
        if self.h:
            self.lib.pdmp3_delete(self.h)
            self.h = None

    def open_feed(self):
        return self.lib.pdmp3_open_feed(self.h)

    def set_quirks(self, iso_mask):
        """pdmp3_amd_set_quirks: PDMP3_ISO_* bits = the standard's behaviour instead of the reference's"""
        self.lib.pdmp3_amd_set_quirks.argtypes = [C.c_void_p, C.c_uint]
        if self.lib.pdmp3_amd_set_quirks(self.h, iso_mask) != 0:
            raise ValueError("pdmp3_amd_set_quirks: unknown bits in %#x" % iso_mask)

    def feed(self, data: bytes):
        buf = (C.c_ubyte * len(data)).from_buffer_copy(data)
        return self.lib.pdmp3_feed(self.h, buf, len(data))

    def read(self, outsize):
        out = (C.c_ubyte * outsize)()
        done = C.c_size_t(0)
        rc = self.lib.pdmp3_read(self.h, out, outsize, C.byref(done))
        return rc, bytes(out[:done.value])

    def decode(self, data: bytes, outsize):
        buf = (C.c_ubyte * max(1, len(data))).from_buffer_copy(data or b"\0")
        out = (C.c_ubyte * outsize)() if outsize else None
        done = C.c_size_t(0)
        rc = self.lib.pdmp3_decode(self.h, buf, len(data), out, outsize, C.byref(done))
        return rc, bytes(out[:done.value]) if outsize else b""

    def getformat(self):
        rate, ch, enc = C.c_long(0), C.c_int(0), C.c_int(0)
        rc = self.lib.pdmp3_getformat(self.h, C.byref(rate), C.byref(ch), C.byref(enc))
        return rc, rate.value, ch.value, enc.value

    def set_encoding(self, enc):
        return self.lib.pdmp3_amd_set_encoding(self.h, enc)

    def set_tap(self, cap_frames):
        self._tap_sp = np.zeros((cap_frames, 2, 2, 576), dtype=np.int16)
        self._tap_sd = np.zeros((cap_frames, 2, 2), dtype=SIDE_DTYPE)
        self.lib.pdmp3_amd_set_tap(self.h, self._tap_sp.ctypes.data_as(C.c_void_p),
                                   self._tap_sd.ctypes.data_as(C.c_void_p), cap_frames)

    def tap(self):
        n = min(self.lib.pdmp3_amd_tap_count(self.h), self._tap_sp.shape[0])
        return self._tap_sp[:n], self._tap_sd[:n]

    def parse_available(self):
        return self.lib.pdmp3_amd_parse_available(self.h)


def stream_loop(mp3, feed_bytes=4096, read_bytes=16384, eager=False, want_pcm=True):
    """pdmp3_amd_stream_loop: the feed / read loop of the reference's driver run in C over a memory buffer.
    -> (PCM bytes delivered, int16 array or None)"""
    lib = load_library()
    lib.pdmp3_amd_stream_loop.restype = C.c_longlong
    lib.pdmp3_amd_stream_loop.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    a = _as_u8(mp3)
    out = np.empty((len(a) // 96 + 8) * 2304, dtype=np.int16) if want_pcm else None
    n = lib.pdmp3_amd_stream_loop(a.ctypes.data_as(C.c_void_p), len(a), out.ctypes.data_as(C.c_void_p) if want_pcm else None,
                                  out.nbytes if want_pcm else 0, feed_bytes, read_bytes, int(eager))
    if n < 0:
        raise RuntimeError("pdmp3_amd_stream_loop: no transform engine")
    return n, (out[:n // 2] if want_pcm else None)


def decode_like_cli(mp3: bytes, dec: "Decoder" = None):
    """The CLI driver loop pdmp3() (pdmp3.c:2552-2587) over a memory buffer."""
    own = dec is None
    if own:
        dec = Decoder()
    dec.open_feed()
    out, pos = [], 0
    while True:
        rc, pcm = dec.read(16384)
        if rc == PDMP3_ERR:
            break
        out.append(pcm)
        if rc == PDMP3_NEED_MORE:
            chunk = mp3[pos:pos + 4096]
            if not chunk:
                break
            dec.feed(chunk)
            pos += len(chunk)
    if own:
        dec.close()
    return b"".join(out)


def parse_like_cli(mp3: bytes, cap_frames, iso=0):
    """Host stage only (no GPU): records the host parser emits when driven with
    the CLI's feed cadence."""
    dec = Decoder(parse_only=True)
    if iso:
        dec.set_quirks(iso)
    dec.set_tap(cap_frames)
    pos = 0
    while True:
        rc = dec.parse_available()
        if rc == PDMP3_ERR:
            break
        chunk = mp3[pos:pos + 4096]
        if not chunk:
            break
        dec.feed(chunk)
        pos += len(chunk)
    sp, sd = dec.tap()
    dec.close()
    return sp.copy(), sd.copy()


def _as_u8(data):
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    return a if a.size else np.zeros(1, dtype=np.uint8)


def _enum(table, value):
    """a name of `table` (None where the table has it) -> its number; a number stays one"""
    return table[value] if isinstance(value, str) or (value is None and None in table) else int(value)


def _window_arg(call, window, win_length):
    """the window / win_length pair of a transform call -> (win_length for the spec, 0 meaning n_fft to the library; the
    window's address or None; the float32 array behind it, to be kept while the spec is in use)"""
    w = None
    if window is not None:
        w = np.ascontiguousarray(window.detach().cpu().numpy() if hasattr(window, "detach") else window, dtype=np.float32)
        if w.ndim != 1 or (win_length is not None and w.size != int(win_length)) or (win_length is None and not w.size):
            raise ValueError("%s: window must hold win_length values" % call)
        win_length = w.size
    return 0 if win_length is None else int(win_length), w.ctypes.data if w is not None else None, w


def _check(spec_of, c_name, sample_rate, kw, refused, *more):
    """every <feature>_check: spec_of(sample_rate=sample_rate, **kw) -> the spec (or (spec, what it points to)); an exception
    of the types `refused` from it is False, any other is the caller's; then the library's verdict (more: its arguments
    behind sample_rate)"""
    try:
        made = spec_of(sample_rate=sample_rate, **kw)
    except refused:
        return False
    spec = made[0] if isinstance(made, tuple) else made        # (made keeps the window alive until the call is over)
    return getattr(load_library(), c_name)(C.byref(spec), int(sample_rate), *[int(m) for m in more]) == 0


def _plan(fn, lead, kinds):
    """fn(*lead, one out-parameter of each ctypes type of `kinds`) -> the tuple of their values"""
    outs = [kind(0) for kind in kinds]
    if fn(*lead, *[C.byref(o) for o in outs]) != 0:
        raise ValueError("%s: bad argument" % fn.__name__)
    return tuple(o.value for o in outs)


_I, _U, _LL = C.c_int, C.c_uint, C.c_longlong


class RingReplay(RuntimeError):
    """PDMP3_BULK_REPLAY: the reference would replay its input ring on this stream (include/pdmp3_bulk.h)"""


class MixedFormat(RuntimeError):
    """PDMP3_BULK_MIXED_FORMAT: a clip's stream changes its sampling frequency or samples per frame: it has no time line in
    samples (include/pdmp3_bulk.h).  .valid / .out: what BulkDecoder.decode_clips_audio would have returned"""


def scan_buffer(mp3, iso=0):
    """(pcm_bytes, frames) the CLI driver would produce for this stream (include/pdmp3_bulk.h); iso: the decoder's switches
    (PDMP3_ISO_LSF changes what counts as a frame)"""
    lib = load_library()
    a = _as_u8(mp3)
    frames = C.c_longlong(0)
    lib.pdmp3_amd_scan_buffer_iso.restype = C.c_longlong
    lib.pdmp3_amd_scan_buffer_iso.argtypes = [C.c_void_p, C.c_size_t, C.c_uint, C.POINTER(C.c_longlong)]
    total = lib.pdmp3_amd_scan_buffer_iso(a.ctypes.data_as(C.c_void_p), len(mp3), iso, C.byref(frames))
    if total == -2:
        raise RingReplay("the reference replays its input ring on this stream (no finite output)")
    return total, frames.value


PDMP3_BULK_REPLAY = -2
PDMP3_BULK_MIXED_FORMAT = -3


def audio_span(rate_in, rate_out, start, n, width=0, rolloff=0.0):
    """pdmp3_amd_audio_span -> (first input sample, count) that output samples [start, start + n) read, unclamped"""
    return _plan(load_library().pdmp3_amd_audio_span, (int(rate_in), int(rate_out), int(width), float(rolloff), int(start), int(n)), (_LL, _LL))


def audio_table(rate_in, rate_out, width=0, rolloff=0.0):
    """pdmp3_amd_audio_table -> (float32 numpy [rows, taps], first tap): row (j M) mod L, tap k on input sample j M // L + first
    tap + k"""
    lib = load_library()
    rows, taps, d0 = C.c_long(0), C.c_int(0), C.c_int(0)
    n = lib.pdmp3_amd_audio_table(int(rate_in), int(rate_out), int(width), float(rolloff), None, 0, C.byref(rows), C.byref(taps), C.byref(d0))
    if n < 0:
        raise ValueError("pdmp3_amd_audio_table: bad argument, equal rates or a table of more than 2^22 coefficients")
    t = np.empty((rows.value, taps.value), dtype=np.float32)
    lib.pdmp3_amd_audio_table(int(rate_in), int(rate_out), int(width), float(rolloff), t.ctypes.data_as(C.c_void_p), t.size, None, None, None)
    return t, d0.value


def audio_lds_plan(rate_in, rate_out, channels, width=0, rolloff=0.0):
    """pdmp3_amd_audio_lds_plan -> (flags, span_cap): what k_clip_audio keeps in LDS for a clip of the pair in a call with
    `channels` channels (flags 1: the input span, 3: the table too, 0: nothing -- every sample straight from memory)"""
    return _plan(load_library().pdmp3_amd_audio_lds_plan, (int(rate_in), int(rate_out), int(width), float(rolloff), int(channels)), (_U, _U))


class _MelSpec(C.Structure):                       # include/pdmp3_bulk.h pdmp3_amd_mel_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("n_fft", C.c_int), ("hop", C.c_int),
                ("n_mels", C.c_int), ("f_min", C.c_double), ("f_max", C.c_double), ("scale", C.c_int), ("norm", C.c_int),
                ("n_frames", C.c_longlong), ("out_mode", C.c_int), ("floor", C.c_double)]


MEL_SCALES = {"slaney": 0, "htk": 1}
MEL_NORMS = {None: 0, "none": 0, "slaney": 1}
MEL_MODES = {"power": 0, "log": 1, "ln": 1, "log10": 2, "whisper": 3}


def _mel_spec(n_frames, sample_rate, n_fft, hop, n_mels, f_min, f_max, scale, norm, mode, floor, channels, width, rolloff):
    return _MelSpec(int(sample_rate), int(channels), int(width), float(rolloff), int(n_fft), int(hop), int(n_mels), float(f_min), float(f_max),
                    _enum(MEL_SCALES, scale), _enum(MEL_NORMS, norm), int(n_frames), _enum(MEL_MODES, mode), float(floor))


def mel_check(sample_rate, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney", mode="log10", floor=1e-10,
              n_frames=1):
    """pdmp3_amd_mel_check -> True when pdmp3_amd_bulk_decode_clips_mel would accept these numbers at sample_rate"""
    kw = dict(n_frames=n_frames, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=f_min, f_max=f_max, scale=scale, norm=norm, mode=mode, floor=floor,
              channels=1, width=0, rolloff=0.0)
    return _check(_mel_spec, "pdmp3_amd_mel_check", sample_rate, kw, ())


def mel_span(n_fft, hop, start, n_frames):
    """pdmp3_amd_mel_span -> (first sample, count) that frames 0 .. n_frames - 1 of a clip at `start` read, unclamped"""
    return _plan(load_library().pdmp3_amd_mel_span, (int(n_fft), int(hop), int(start), int(n_frames)), (_LL, _LL))


def mel_dft_table(n_fft):
    """pdmp3_amd_mel_dft_table -> float32 numpy [rows, 2 Kp] as k_clip_mel reads it: row n, w[n] cos at column k, -w[n] sin at
    column Kp + k, zeros in the padding"""
    lib = load_library()
    rows, cols = C.c_int(0), C.c_int(0)
    if lib.pdmp3_amd_mel_dft_table(int(n_fft), None, 0, C.byref(rows), C.byref(cols)) < 0:
        raise ValueError("pdmp3_amd_mel_dft_table: n_fft must be even, 16 .. 1024")
    t = np.full((rows.value, cols.value), np.nan, dtype=np.float32)
    lib.pdmp3_amd_mel_dft_table(int(n_fft), t.ctypes.data_as(C.c_void_p), t.size, None, None)
    return t


def mel_filterbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney"):
    """pdmp3_amd_mel_filterbank -> float32 numpy [n_mels, n_fft // 2 + 1]"""
    lib = load_library()
    sc, no = _enum(MEL_SCALES, scale), _enum(MEL_NORMS, norm)
    n = lib.pdmp3_amd_mel_filterbank(int(sample_rate), int(n_fft), int(n_mels), float(f_min), float(f_max), sc, no, None, 0)
    if n < 0:
        raise ValueError("pdmp3_amd_mel_filterbank: bad argument")
    w = np.full((int(n_mels), int(n_fft) // 2 + 1), np.nan, dtype=np.float32)
    lib.pdmp3_amd_mel_filterbank(int(sample_rate), int(n_fft), int(n_mels), float(f_min), float(f_max), sc, no, w.ctypes.data_as(C.c_void_p), w.size)
    return w


def mel_tile(n_fft, hop, n_mels):
    """pdmp3_amd_mel_tile -> (frames of a workgroup of k_clip_mel, LDS floats between two hops, LDS bytes of a workgroup)"""
    return _plan(load_library().pdmp3_amd_mel_tile, (int(n_fft), int(hop), int(n_mels)), (_I, _I, _U))


class _FbankSpec(C.Structure):                     # include/pdmp3_bulk.h pdmp3_amd_fbank_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("win_length", C.c_int), ("hop", C.c_int),
                ("n_mels", C.c_int), ("round_to_power_of_two", C.c_int), ("remove_dc_offset", C.c_int), ("preemphasis", C.c_double),
                ("window", C.c_int), ("blackman_coeff", C.c_double), ("low_freq", C.c_double), ("high_freq", C.c_double), ("out_mode", C.c_int),
                ("use_energy", C.c_int), ("htk_compat", C.c_int), ("energy_floor", C.c_double), ("subtract_mean", C.c_int), ("scale", C.c_double),
                ("n_frames", C.c_longlong), ("dither", C.c_double), ("vtln_warp", C.c_double), ("no_power", C.c_int), ("no_raw_energy", C.c_int),
                ("no_snip_edges", C.c_int)]


FBANK_WINDOWS = {"povey": 0, "hanning": 1, "hamming": 2, "rectangular": 3, "blackman": 4}


def _fbank_spec(n_frames=1, sample_rate=16000, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, win_length=None, hop=None,
                round_to_power_of_two=True, remove_dc_offset=True, preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42,
                low_freq=20.0, high_freq=0.0, use_log_fbank=True, use_energy=False, htk_compat=False, energy_floor=1.0, subtract_mean=False,
                scale=1.0, channels=1, width=0, rolloff=0.0, dither=0.0, use_power=True, raw_energy=True, snip_edges=True, vtln_warp=1.0):
    """torchaudio.compliance.kaldi.fbank's arguments -> pdmp3_amd_fbank_spec.  Nw = int(sample_rate * frame_length * 0.001) as
    Kaldi computes it, hop likewise; win_length / hop in samples override them.  An unknown window_type gives one the check
    refuses.  sample_rate 0 (the clips' own rate) needs win_length and hop."""
    sr = int(sample_rate)
    nw = int(win_length) if win_length is not None else int(sr * frame_length * 0.001)
    h = int(hop) if hop is not None else int(sr * frame_shift * 0.001)
    win = FBANK_WINDOWS.get(window_type, -1) if isinstance(window_type, str) else int(window_type)
    return _FbankSpec(sr, int(channels), int(width), float(rolloff), nw, h, int(num_mel_bins), int(bool(round_to_power_of_two)),
                      int(bool(remove_dc_offset)), float(preemphasis_coefficient), win, float(blackman_coeff), float(low_freq), float(high_freq),
                      int(use_log_fbank) if isinstance(use_log_fbank, (bool, int)) else -1, int(bool(use_energy)), int(bool(htk_compat)),
                      float(energy_floor), int(bool(subtract_mean)), float(scale), int(n_frames), float(dither), float(vtln_warp),
                      int(not use_power), int(not raw_energy), int(not snip_edges))


def fbank_check(sample_rate=16000, **kw):
    """pdmp3_amd_fbank_check -> True when pdmp3_amd_bulk_decode_clips_fbank would accept these arguments (decode_clips_fbank's,
    and dither / use_power / raw_energy / snip_edges / vtln_warp, which are refused unless they have torchaudio's defaults)"""
    return _check(_fbank_spec, "pdmp3_amd_fbank_check", sample_rate, kw, ())


def fbank_dft_length(win_length, round_to_power_of_two=True):
    """pdmp3_amd_fbank_dft_length -> N"""
    n = load_library().pdmp3_amd_fbank_dft_length(int(win_length), int(bool(round_to_power_of_two)))
    if n < 0:
        raise ValueError("pdmp3_amd_fbank_dft_length: win_length must be 2 .. 1024, and even without round_to_power_of_two")
    return n


def fbank_table(win_length=400, round_to_power_of_two=True, remove_dc_offset=True, preemphasis_coefficient=0.97, window_type="povey",
                blackman_coeff=0.42, scale=1.0):
    """pdmp3_amd_fbank_table -> float32 numpy [Nw rounded up to 4, 2 Kp] as k_clip_fbank reads it: DC removal, pre-emphasis, the
    window, the zero padding to N and `scale` folded into the DFT; Re at column k, Im at Kp + k, zeros in the padding"""
    lib = load_library()
    spec = _fbank_spec(win_length=win_length, hop=1, round_to_power_of_two=round_to_power_of_two, remove_dc_offset=remove_dc_offset,
                       preemphasis_coefficient=preemphasis_coefficient, window_type=window_type, blackman_coeff=blackman_coeff, scale=scale)
    rows, cols = C.c_int(0), C.c_int(0)
    if lib.pdmp3_amd_fbank_table(C.byref(spec), None, 0, C.byref(rows), C.byref(cols)) < 0:
        raise ValueError("pdmp3_amd_fbank_table: bad argument")
    t = np.full((rows.value, cols.value), np.nan, dtype=np.float32)
    lib.pdmp3_amd_fbank_table(C.byref(spec), t.ctypes.data_as(C.c_void_p), t.size, None, None)
    return t


def fbank_filterbank(sample_rate, n_dft, num_mel_bins, low_freq=20.0, high_freq=0.0):
    """pdmp3_amd_fbank_filterbank -> float32 numpy [num_mel_bins, n_dft // 2]"""
    lib = load_library()
    n = lib.pdmp3_amd_fbank_filterbank(int(sample_rate), int(n_dft), int(num_mel_bins), float(low_freq), float(high_freq), None, 0)
    if n < 0:
        raise ValueError("pdmp3_amd_fbank_filterbank: bad argument")
    w = np.full((int(num_mel_bins), int(n_dft) // 2), np.nan, dtype=np.float32)
    lib.pdmp3_amd_fbank_filterbank(int(sample_rate), int(n_dft), int(num_mel_bins), float(low_freq), float(high_freq), w.ctypes.data_as(C.c_void_p), w.size)
    return w


def fbank_valid(n_out, start, win_length, hop, n_frames):
    """pdmp3_amd_fbank_valid -> the frames of a clip at `start` that lie wholly inside a stream of n_out samples"""
    v = load_library().pdmp3_amd_fbank_valid(int(n_out), int(start), int(win_length), int(hop), int(n_frames))
    if v < 0:
        raise ValueError("pdmp3_amd_fbank_valid: bad argument")
    return v


def fbank_tile(win_length, n_dft, hop, num_mel_bins):
    """pdmp3_amd_fbank_tile -> (frames of a workgroup of k_clip_fbank, LDS floats between two hops, LDS bytes of a workgroup;
    more than 64 KB: the static-array kernel)"""
    return _plan(load_library().pdmp3_amd_fbank_tile, (int(win_length), int(n_dft), int(hop), int(num_mel_bins)), (_I, _I, _U))


class _MfccSpec(C.Structure):                      # include/pdmp3_bulk.h pdmp3_amd_mfcc_spec
    _fields_ = [("fbank", _FbankSpec), ("num_ceps", C.c_int), ("cepstral_lifter", C.c_double)]


def _mfcc_spec(num_ceps=13, cepstral_lifter=22.0, **kw):
    """torchaudio.compliance.kaldi.mfcc's arguments -> pdmp3_amd_mfcc_spec (the filterbank's through _fbank_spec; a
    cepstral_lifter that is no number gives one the check refuses)"""
    try:
        q = float(cepstral_lifter)
    except (TypeError, ValueError):
        q = float("nan")
    return _MfccSpec(_fbank_spec(**kw), int(num_ceps), q)


def mfcc_check(sample_rate=16000, **kw):
    """pdmp3_amd_mfcc_check -> True when pdmp3_amd_bulk_decode_clips_mfcc would accept these arguments (decode_clips_mfcc's,
    and use_log_fbank / dither / use_power / raw_energy / snip_edges / vtln_warp, which are refused unless they have
    torchaudio's defaults)"""
    return _check(_mfcc_spec, "pdmp3_amd_mfcc_check", sample_rate, kw, ())


def mfcc_dct_table(num_mel_bins=23, num_ceps=13, cepstral_lifter=22.0, htk_compat=False, use_energy=False):
    """pdmp3_amd_mfcc_dct_table -> float32 numpy [num_mel_bins rounded up to 16, num_ceps rounded up to 16] as k_clip_mfcc reads
    it: the orthonormal DCT-II rows with the lifter, htk_compat's sqrt 2 and the column order folded in; zeros in the column
    that holds the energy and in the padding"""
    lib = load_library()
    spec = _mfcc_spec(num_ceps, cepstral_lifter, num_mel_bins=num_mel_bins, htk_compat=htk_compat, use_energy=use_energy)
    rows, cols = C.c_int(0), C.c_int(0)
    if lib.pdmp3_amd_mfcc_dct_table(C.byref(spec), None, 0, C.byref(rows), C.byref(cols)) < 0:
        raise ValueError("pdmp3_amd_mfcc_dct_table: bad argument")
    t = np.full((rows.value, cols.value), np.nan, dtype=np.float32)
    lib.pdmp3_amd_mfcc_dct_table(C.byref(spec), t.ctypes.data_as(C.c_void_p), t.size, None, None)
    return t


def mfcc_tile(win_length, n_dft, hop, num_mel_bins, num_ceps):
    """pdmp3_amd_mfcc_tile -> (frames of a workgroup of k_clip_mfcc, LDS floats between two hops, LDS bytes of a workgroup;
    more than 64 KB: the static-array kernel)"""
    return _plan(load_library().pdmp3_amd_mfcc_tile, (int(win_length), int(n_dft), int(hop), int(num_mel_bins), int(num_ceps)), (_I, _I, _U))


class _StftSpec(C.Structure):                      # include/pdmp3_bulk.h pdmp3_amd_stft_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("n_fft", C.c_int), ("hop", C.c_int),
                ("win_length", C.c_int), ("window", C.c_void_p), ("normalized", C.c_int), ("n_frames", C.c_longlong), ("out_mode", C.c_int),
                ("floor", C.c_double)]


STFT_MODES = {"complex": 0, "magnitude": 1, "power": 2, "log": 3, "ln": 3, "log10": 4}


def _stft_spec(n_frames=1, sample_rate=16000, n_fft=400, hop=160, win_length=None, window=None, normalized=False, mode="complex", floor=1e-10,
               channels=1, width=0, rolloff=0.0):
    """-> (spec, the float32 array its window points to, to be kept while the spec is in use)"""
    nw, wp, w = _window_arg("stft", window, win_length)
    spec = _StftSpec(int(sample_rate), int(channels), int(width), float(rolloff), int(n_fft), int(hop), nw, wp, int(bool(normalized)), int(n_frames),
                     _enum(STFT_MODES, mode), float(floor))
    return spec, w


def stft_check(sample_rate=16000, **kw):
    """pdmp3_amd_stft_check -> True when pdmp3_amd_bulk_decode_clips_stft would accept these numbers (decode_clips_stft's
    argument names) at sample_rate"""
    return _check(_stft_spec, "pdmp3_amd_stft_check", sample_rate, kw, (ValueError, KeyError))


def stft_table(n_fft=400, win_length=None, window=None, normalized=False):
    """pdmp3_amd_stft_table -> float32 numpy [rows, 2 Kp] as k_clip_stft reads it: row n, s w[n] cos at column k, -s w[n] sin at
    column Kp + k, zeros outside the window's support and in the padding"""
    lib = load_library()
    spec, keep = _stft_spec(n_fft=n_fft, win_length=win_length, window=window, normalized=normalized)
    rows, cols = C.c_int(0), C.c_int(0)
    if lib.pdmp3_amd_stft_table(C.byref(spec), None, 0, C.byref(rows), C.byref(cols)) < 0:
        raise ValueError("pdmp3_amd_stft_table: bad argument")
    t = np.full((rows.value, cols.value), np.nan, dtype=np.float32)
    lib.pdmp3_amd_stft_table(C.byref(spec), t.ctypes.data_as(C.c_void_p), t.size, None, None)
    return t


def stft_tile(n_fft, hop, mode="complex"):
    """pdmp3_amd_stft_tile -> (frames of a workgroup of k_clip_stft, LDS floats between two hops, LDS bytes of a workgroup)"""
    return _plan(load_library().pdmp3_amd_stft_tile, (int(n_fft), int(hop), _enum(STFT_MODES, mode)), (_I, _I, _U))


class _CqtSpec(C.Structure):                       # include/pdmp3_bulk.h pdmp3_amd_cqt_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("hop", C.c_int), ("fmin", C.c_double),
                ("n_bins", C.c_int), ("bins_per_octave", C.c_int), ("filter_scale", C.c_double), ("norm", C.c_int), ("scale", C.c_int),
                ("n_frames", C.c_longlong), ("out_mode", C.c_int), ("floor", C.c_double)]


CQT_FMIN = 32.70319566257483                       # C1


def _cqt_spec(n_frames=1, sample_rate=22050, hop=512, fmin=CQT_FMIN, n_bins=84, bins_per_octave=12, filter_scale=1.0, norm=1, scale=1,
              mode="magnitude", floor=1e-10, channels=1, width=0, rolloff=0.0):
    return _CqtSpec(int(sample_rate), int(channels), int(width), float(rolloff), int(hop), float(fmin), int(n_bins), int(bins_per_octave),
                    float(filter_scale), int(norm), int(scale), int(n_frames), _enum(STFT_MODES, mode), float(floor))


def cqt_check(sample_rate=22050, **kw):
    """pdmp3_amd_cqt_check -> True when pdmp3_amd_bulk_decode_clips_cqt would accept these numbers (decode_clips_cqt's argument
    names) at sample_rate"""
    return _check(_cqt_spec, "pdmp3_amd_cqt_check", sample_rate, kw, (ValueError, KeyError, OverflowError))


def cqt_lengths(sample_rate=22050, **kw):
    """pdmp3_amd_cqt_lengths -> (f_k float64 [n_bins], h_k int32 [n_bins]): the bins' frequencies and half lengths, N_k = 2 h_k + 1"""
    spec = _cqt_spec(sample_rate=sample_rate, **kw)
    n = max(spec.n_bins, 1)
    f = np.full(n, np.nan, dtype=np.float64)
    h = np.full(n, -1, dtype=np.int32)
    if load_library().pdmp3_amd_cqt_lengths(C.byref(spec), int(sample_rate), f.ctypes.data, h.ctypes.data, n) != spec.n_bins:
        raise ValueError("pdmp3_amd_cqt_lengths: bad argument")
    return f, h


def cqt_table(sample_rate=22050, **kw):
    """pdmp3_amd_cqt_table -> (float32 numpy [rows, 32] as k_clip_cqt reads it, rows of each tile of 16 bins, first row of each):
    tile t's row r holds Re's coefficient of bin 16 t + j at sample m = r - h_(16 t) in column j and Im's in column 16 + j"""
    lib = load_library()
    spec = _cqt_spec(sample_rate=sample_rate, **kw)
    nt = (max(spec.n_bins, 1) + 15) // 16
    rows = np.zeros(nt, dtype=np.int32)
    at = np.zeros(nt, dtype=np.int32)
    count = lib.pdmp3_amd_cqt_table(C.byref(spec), int(sample_rate), None, 0, rows.ctypes.data, at.ctypes.data)
    if count < 0:
        raise ValueError("pdmp3_amd_cqt_table: bad argument")
    t = np.full((count // 32, 32), np.nan, dtype=np.float32)
    if lib.pdmp3_amd_cqt_table(C.byref(spec), int(sample_rate), t.ctypes.data, t.size, None, None) != count:
        raise ValueError("pdmp3_amd_cqt_table: bad argument")
    return t, rows, at


def cqt_plan(sample_rate=22050, **kw):
    """pdmp3_amd_cqt_plan -> (frames of a workgroup of k_clip_cqt, LDS floats between two hops, LDS bytes of a workgroup, rows
    from which a tile is split, segments of a split tile, tiles that are split)"""
    spec = _cqt_spec(sample_rate=sample_rate, **kw)
    return _plan(load_library().pdmp3_amd_cqt_plan, (C.byref(spec), int(sample_rate)), (_I, _I, _U, _I, _I, _I))


class _ChromaSpec(C.Structure):                    # include/pdmp3_bulk.h pdmp3_amd_chroma_spec
    _fields_ = [("cqt", _CqtSpec), ("n_chroma", C.c_int), ("base_class", C.c_int), ("chroma_norm", C.c_int), ("norm_floor", C.c_double)]


CHROMA_NORMS = {None: 0, "none": 0, "l1": 1, "l2": 2, "max": 3, "inf": 3}


def _chroma_spec(n_frames=1, sample_rate=22050, hop=512, fmin=CQT_FMIN, n_bins=84, bins_per_octave=12, n_chroma=12, base_class=0, filter_scale=1.0,
                 norm=1, scale=1, quantity="magnitude", chroma_norm="max", norm_floor=1e-10, channels=1, width=0, rolloff=0.0):
    q = _enum(STFT_MODES, quantity)
    if isinstance(chroma_norm, str) and chroma_norm not in CHROMA_NORMS:
        raise ValueError("chroma_norm is one of %s" % sorted(k for k in CHROMA_NORMS if k))
    cn = _enum(CHROMA_NORMS, chroma_norm)
    cqt = _cqt_spec(n_frames, sample_rate, hop, fmin, n_bins, bins_per_octave, filter_scale, norm, scale, q, 0.0, channels, width, rolloff)
    return _ChromaSpec(cqt, int(n_chroma), int(base_class), cn, float(norm_floor))


def chroma_check(sample_rate=22050, **kw):
    """pdmp3_amd_chroma_check -> True when pdmp3_amd_bulk_decode_clips_chroma would accept these numbers (decode_clips_chroma's
    argument names) at sample_rate"""
    return _check(_chroma_spec, "pdmp3_amd_chroma_check", sample_rate, kw, (ValueError, KeyError, OverflowError))


def chroma_map(sample_rate=22050, **kw):
    """pdmp3_amd_chroma_map -> (class of every bin int32 [n_bins], bins of every class int32 [n_chroma])"""
    spec = _chroma_spec(sample_rate=sample_rate, **kw)
    cls = np.full(max(spec.cqt.n_bins, 1), -1, dtype=np.int32)
    count = np.full(max(min(spec.n_chroma, 4096), 1), -1, dtype=np.int32)
    if load_library().pdmp3_amd_chroma_map(C.byref(spec), int(sample_rate), cls.ctypes.data, cls.size, count.ctypes.data) != spec.cqt.n_bins:
        raise ValueError("pdmp3_amd_chroma_map: bad argument")
    return cls, count


def chroma_plan(sample_rate=22050, **kw):
    """pdmp3_amd_chroma_plan -> (frames of a workgroup of k_clip_chroma, LDS floats between two hops, LDS bytes of a workgroup,
    rows from which a tile is split, segments of a split tile, tiles that are split, LDS floats in front of the q plane, LDS
    floats in front of the class plane)"""
    spec = _chroma_spec(sample_rate=sample_rate, **kw)
    return _plan(load_library().pdmp3_amd_chroma_plan, (C.byref(spec), int(sample_rate)), (_I, _I, _U, _I, _I, _I, _U, _U))


def stft_long_check(sample_rate=44100, n_fft=2048, hop=512, **kw):
    """pdmp3_amd_stft_long_check -> True when pdmp3_amd_bulk_decode_clips_stft_long would accept these numbers
    (decode_clips_stft_long's argument names) at sample_rate"""
    return _check(_stft_spec, "pdmp3_amd_stft_long_check", sample_rate, dict(kw, n_fft=n_fft, hop=hop), (ValueError, KeyError))


def stft_long_tables(n_fft=2048, win_length=None, window=None, normalized=False):
    """pdmp3_amd_stft_long_tables -> the four float32 tables of the two-stage transform as k_clip_stft_long reads them:
    (wt [N], the 64-point DFT [64, 128], the N2-point half DFT [2 N2, N2], the twiddles [N2, 128]), N2 = n_fft // 64"""
    lib = load_library()
    spec, keep = _stft_spec(n_fft=n_fft, hop=n_fft, win_length=win_length, window=window, normalized=normalized)
    shapes = (C.c_int * 8)()
    count = lib.pdmp3_amd_stft_long_tables(C.byref(spec), None, 0, shapes)
    if count < 0:
        raise ValueError("pdmp3_amd_stft_long_tables: bad argument")
    t = np.full(count, np.nan, dtype=np.float32)
    lib.pdmp3_amd_stft_long_tables(C.byref(spec), t.ctypes.data_as(C.c_void_p), t.size, None)
    out, at = [], 0
    for i in range(4):
        n = shapes[2 * i] * shapes[2 * i + 1]
        out.append(t[at:at + n].reshape((shapes[2 * i], shapes[2 * i + 1]) if i else (n,)))
        at += n
    assert at == count
    return tuple(out)


def stft_long_plan(n_fft, hop, mode="complex"):
    """pdmp3_amd_stft_long_plan -> (frames of a workgroup of k_clip_stft_long, 0, LDS bytes of a workgroup)"""
    return _plan(load_library().pdmp3_amd_stft_long_plan, (int(n_fft), int(hop), _enum(STFT_MODES, mode)), (_I, _I, _U))


class _MelLongSpec(C.Structure):                   # include/pdmp3_bulk.h pdmp3_amd_mel_long_spec
    _fields_ = [("mel", _MelSpec), ("win_length", C.c_int), ("window", C.c_void_p)]


def _mel_long_spec(n_frames=1, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney",
                   mode="log10", floor=1e-10, win_length=None, window=None, channels=1, width=0, rolloff=0.0):
    """-> (spec, the float32 array its window points to, to be kept while the spec is in use)"""
    nw, wp, w = _window_arg("mel_long", window, win_length)
    mel = _mel_spec(n_frames, sample_rate, n_fft, hop, n_mels, f_min, f_max, scale, norm, mode, floor, channels, width, rolloff)
    return _MelLongSpec(mel, nw, wp), w


def mel_long_check(sample_rate=22050, **kw):
    """pdmp3_amd_mel_long_check -> True when pdmp3_amd_bulk_decode_clips_mel_long would accept these numbers
    (decode_clips_mel_long's argument names) at sample_rate"""
    return _check(_mel_long_spec, "pdmp3_amd_mel_long_check", sample_rate, kw, (ValueError, KeyError))


def _mel_long_bank(sample_rate, n_fft, n_mels, f_min, f_max, scale, norm):
    sc, no = _enum(MEL_SCALES, scale), _enum(MEL_NORMS, norm)
    return int(sample_rate), int(n_fft), int(n_mels), float(f_min), float(f_max), sc, no


def mel_long_filterbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney"):
    """pdmp3_amd_mel_long_filterbank -> float32 numpy [n_mels, n_fft // 2 + 1]"""
    lib = load_library()
    a = _mel_long_bank(sample_rate, n_fft, n_mels, f_min, f_max, scale, norm)
    if lib.pdmp3_amd_mel_long_filterbank(*a, None, 0) < 0:
        raise ValueError("pdmp3_amd_mel_long_filterbank: bad argument")
    w = np.full((int(n_mels), int(n_fft) // 2 + 1), np.nan, dtype=np.float32)
    lib.pdmp3_amd_mel_long_filterbank(*a, w.ctypes.data_as(C.c_void_p), w.size)
    return w


def mel_long_operand(sample_rate, n_fft, n_mels, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney"):
    """pdmp3_amd_mel_long_operand -> float32 numpy [n_fft // 2, n_mels rounded up to 16]: the filterbank as k_clip_mel_long
    reads it, the bins' rows in the kernel's order"""
    lib = load_library()
    a = _mel_long_bank(sample_rate, n_fft, n_mels, f_min, f_max, scale, norm)
    rows, cols = C.c_int(0), C.c_int(0)
    if lib.pdmp3_amd_mel_long_operand(*a, None, 0, C.byref(rows), C.byref(cols)) < 0:
        raise ValueError("pdmp3_amd_mel_long_operand: bad argument")
    op = np.full((rows.value, cols.value), np.nan, dtype=np.float32)
    lib.pdmp3_amd_mel_long_operand(*a, op.ctypes.data_as(C.c_void_p), op.size, None, None)
    return op


def mel_long_plan(n_fft, hop, n_mels):
    """pdmp3_amd_mel_long_plan -> (frames of a workgroup of k_clip_mel_long, 0, LDS bytes of a workgroup)"""
    return _plan(load_library().pdmp3_amd_mel_long_plan, (int(n_fft), int(hop), int(n_mels)), (_I, _I, _U))


class _SpectralSpec(C.Structure):                  # include/pdmp3_bulk.h pdmp3_amd_spectral_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("n_fft", C.c_int), ("hop", C.c_int),
                ("win_length", C.c_int), ("window", C.c_void_p), ("n_frames", C.c_longlong), ("roll_percent", C.c_double), ("amin", C.c_double),
                ("zcr_threshold", C.c_double)]


SPECTRAL_ROWS = ("rms", "zcr", "centroid", "bandwidth", "rolloff", "flatness")


def _spectral_spec(n_frames=1, sample_rate=22050, n_fft=2048, hop=512, roll_percent=0.85, amin=1e-10, zcr_threshold=1e-10, channels=1,
                   win_length=None, window=None, width=0, rolloff=0.0):
    """-> (spec, the float32 array its window points to, to be kept while the spec is in use)"""
    nw, wp, w = _window_arg("spectral", window, win_length)
    spec = _SpectralSpec(int(sample_rate), int(channels), int(width), float(rolloff), int(n_fft), int(hop), nw, wp, int(n_frames),
                         float(roll_percent), float(amin), float(zcr_threshold))
    return spec, w


def spectral_check(sample_rate=22050, **kw):
    """pdmp3_amd_spectral_check -> True when pdmp3_amd_bulk_decode_clips_spectral would accept these numbers
    (decode_clips_spectral's argument names) at sample_rate"""
    return _check(_spectral_spec, "pdmp3_amd_spectral_check", sample_rate, kw, (ValueError, KeyError, TypeError, OverflowError))


def spectral_plan(n_fft, hop):
    """pdmp3_amd_spectral_plan -> (frames of a workgroup of k_clip_spectral, 0, LDS bytes of a workgroup)"""
    return _plan(load_library().pdmp3_amd_spectral_plan, (int(n_fft), int(hop)), (_I, _I, _U))


class _HpssSpec(C.Structure):                      # include/pdmp3_bulk.h pdmp3_amd_hpss_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("n_fft", C.c_int), ("hop", C.c_int),
                ("win_length", C.c_int), ("window", C.c_void_p), ("n_frames", C.c_longlong), ("kernel_harm", C.c_int), ("kernel_perc", C.c_int),
                ("margin_harm", C.c_double), ("margin_perc", C.c_double), ("power", C.c_double), ("out_mode", C.c_int)]


HPSS_MODES = {"mask": 0, "magnitude": 1, "complex": 2, "median": 3}


def _hpss_spec(n_frames=1, sample_rate=22050, n_fft=2048, hop=512, kernel_size=31, power=2.0, margin=1.0, mode="mask", channels=1,
               win_length=None, window=None, width=0, rolloff=0.0):
    """-> (spec, the float32 array its window points to, to be kept while the spec is in use); kernel_size and margin: one
    number or (harmonic, percussive), as librosa takes them"""
    nw, wp, w = _window_arg("hpss", window, win_length)
    kh, kp = kernel_size if isinstance(kernel_size, (tuple, list)) else (kernel_size, kernel_size)
    mh, mp = margin if isinstance(margin, (tuple, list)) else (margin, margin)
    if int(kh) != kh or int(kp) != kp:
        raise ValueError("hpss: kernel sizes are integers")
    spec = _HpssSpec(int(sample_rate), int(channels), int(width), float(rolloff), int(n_fft), int(hop), nw, wp, int(n_frames), int(kh), int(kp),
                     float(mh), float(mp), float(power), _enum(HPSS_MODES, mode))
    return spec, w


def hpss_check(sample_rate=22050, **kw):
    """pdmp3_amd_hpss_check -> True when pdmp3_amd_bulk_decode_clips_hpss would accept these numbers (decode_clips_hpss's
    argument names) at sample_rate"""
    return _check(_hpss_spec, "pdmp3_amd_hpss_check", sample_rate, kw, (ValueError, KeyError, TypeError, OverflowError))


def hpss_plan(kernel_harm=31, kernel_perc=31):
    """pdmp3_amd_hpss_plan -> (frames in front, frames behind, bins of a workgroup of k_clip_hpss, its frames, the floats between
    two rows of its tile in LDS, its LDS bytes)"""
    return _plan(load_library().pdmp3_amd_hpss_plan, (int(kernel_harm), int(kernel_perc)), (_I,) * 5 + (_U,))


class _MfccLongSpec(C.Structure):                  # include/pdmp3_bulk.h pdmp3_amd_mfcc_long_spec
    _fields_ = [("mel", _MelLongSpec), ("top_db", C.c_double), ("n_mfcc", C.c_int), ("lifter", C.c_double), ("deltas", C.c_int),
                ("delta_width", C.c_int), ("out_mode", C.c_int)]


MFCC_LONG_MODES = {"mfcc": 0, "db": 1}


def _mfcc_long_spec(n_frames=1, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, n_mfcc=20, lifter=0.0, top_db=80.0, amin=1e-10, deltas=0,
                    delta_width=9, out_mode="mfcc", f_min=0.0, f_max=0.0, scale="slaney", norm="slaney", win_length=None, window=None, channels=1,
                    width=0, rolloff=0.0):
    """-> (spec, what its window points to).  top_db None: no clamp (a negative value to the library)"""
    mel, keep = _mel_long_spec(n_frames, sample_rate, n_fft, hop, n_mels, f_min, f_max, scale, norm, "log10", amin, win_length, window, channels,
                               width, rolloff)
    mode = _enum(MFCC_LONG_MODES, out_mode)
    if mode == 1:                                         # (the dB mode reads none of the cepstral fields)
        n_mfcc, lifter, deltas, delta_width = 0, 0.0, 0, 0
    elif int(n_mfcc) != n_mfcc or int(deltas) != deltas or int(delta_width) != delta_width:
        raise ValueError("mfcc_long: n_mfcc, deltas and delta_width are integers")
    if top_db is not None and float(top_db) < 0.0:
        raise ValueError("mfcc_long: top_db is None or not negative")
    top = -1.0 if top_db is None else float(top_db)
    return _MfccLongSpec(mel, top, int(n_mfcc), float(lifter), int(deltas), int(delta_width), mode), keep


def mfcc_long_check(sample_rate=22050, **kw):
    """pdmp3_amd_mfcc_long_check -> True when pdmp3_amd_bulk_decode_clips_mfcc_long would accept these numbers
    (decode_clips_mfcc_long's argument names) at sample_rate"""
    return _check(_mfcc_long_spec, "pdmp3_amd_mfcc_long_check", sample_rate, kw, (ValueError, KeyError, OverflowError, TypeError))


def mfcc_long_dct_table(n_mels=128, n_mfcc=20, lifter=0.0):
    """pdmp3_amd_mfcc_long_dct_table -> float32 numpy [n_mfcc rounded up to 16, n_mels rounded up to 16]: the orthonormal
    DCT-II with librosa's lifter folded in as k_clip_mfcc_long reads it, zeros in the padding"""
    lib = load_library()
    rows, cols = C.c_int(0), C.c_int(0)
    if lib.pdmp3_amd_mfcc_long_dct_table(int(n_mels), int(n_mfcc), float(lifter), None, 0, C.byref(rows), C.byref(cols)) < 0:
        raise ValueError("pdmp3_amd_mfcc_long_dct_table: bad argument")
    t = np.full((rows.value, cols.value), np.nan, dtype=np.float32)
    lib.pdmp3_amd_mfcc_long_dct_table(int(n_mels), int(n_mfcc), float(lifter), t.ctypes.data_as(C.c_void_p), t.size, None, None)
    return t


def mfcc_long_delta_taps(delta_width=9):
    """pdmp3_amd_mfcc_long_delta_taps -> float64 numpy [2, delta_width]: the taps of the first and the second delta, j ascending"""
    w = int(delta_width)
    t = np.full((2, max(w, 1)), np.nan, dtype=np.float64)
    if load_library().pdmp3_amd_mfcc_long_delta_taps(w, t.ctypes.data_as(C.c_void_p), t.size) != w:
        raise ValueError("pdmp3_amd_mfcc_long_delta_taps: delta_width must be odd, 3 .. 17")
    return t


def mfcc_long_plan(n_mels=128, n_mfcc=20, deltas=0, delta_width=9, out_mode="mfcc"):
    """pdmp3_amd_mfcc_long_plan -> (log-mel frames in front of frame 0, behind the last frame, frames of a workgroup of
    k_clip_mfcc_long, the floats between two rows of its plane of dB values, of its plane of cepstra, its LDS bytes)"""
    return _plan(load_library().pdmp3_amd_mfcc_long_plan, (int(n_mels), int(n_mfcc), int(deltas), int(delta_width), _enum(MFCC_LONG_MODES, out_mode)),
                 (_I,) * 5 + (_U,))


class StreamIndex:
    """include/pdmp3_bulk.h pdmp3_amd_index: what a stream's frames are and where their PCM lies in the whole-stream output,
    built once, for BulkDecoder.decode_range / decode_clips.  .frames (PDMP3_BULK_REPLAY when the scan ends in a ring replay),
    .pcm_offsets (numpy int64, frames + 1 entries: bytes of the whole-stream output in front of each frame), .split (the
    split scan's pre-pass took the stream: clips are scanned from its snapshots; False: from frame 0).  iso: the decoder's
    switches (only ISO_LSF matters); spacing: frames between snapshots (0: the library's default).  The index does not keep
    the stream: the decode calls are given the same bytes."""

    def __init__(self, mp3, iso=0, spacing=0):
        self.lib = load_library()
        a = _as_u8(mp3)
        self.n = len(mp3)
        self.iso = iso
        self.h = self.lib.pdmp3_amd_index_new_spacing(a.ctypes.data_as(C.c_void_p), len(mp3), iso, int(spacing))
        if not self.h:
            raise MemoryError("pdmp3_amd_index_new failed")
        self.frames = self.lib.pdmp3_amd_index_frames(self.h)
        self.replay = self.frames == PDMP3_BULK_REPLAY
        self.split = bool(self.lib.pdmp3_amd_index_split(self.h))
        # the stream's format (clips by sample position): one_format False = its frames differ in rate or samples per frame
        rate, ch, spf = C.c_long(0), C.c_int(0), C.c_int(0)
        self.one_format = self.lib.pdmp3_amd_index_format(self.h, C.byref(rate), C.byref(ch), C.byref(spf)) == 1
        self.rate, self.channels, self.frame_samples = rate.value, ch.value, spf.value
        self.samples = self.lib.pdmp3_amd_index_samples(self.h)
        self.pcm_offsets = None
        if not self.replay:
            self.pcm_offsets = np.empty(self.frames + 1, dtype=np.int64)
            self.lib.pdmp3_amd_index_pcm_offsets(self.h, self.pcm_offsets.ctypes.data_as(C.c_void_p), self.frames + 1)

    def clamp(self, first, count):
        """the range [a, b) a clip of (first, count) stands for"""
        a = min(max(int(first), 0), self.frames)
        return a, a + min(max(int(count), 0), self.frames - a)

    def close(self):
        if self.h:
            self.lib.pdmp3_amd_index_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:                          # noqa: BLE001  (interpreter shutdown)
            pass


def _int16_buffer(o, ndim):
    """(address, bytes) of a contiguous int16 numpy array or torch tensor"""
    if hasattr(o, "data_ptr"):
        assert o.dim() == ndim and o.is_contiguous() and o.element_size() == 2
        return o.data_ptr(), o.numel() * 2
    assert o.ndim == ndim and o.flags["C_CONTIGUOUS"] and o.dtype == np.int16
    return o.ctypes.data, o.nbytes


class _Clip(C.Structure):                          # include/pdmp3_bulk.h pdmp3_amd_clip
    _fields_ = [("mp3", C.c_void_p), ("n", C.c_size_t), ("index", C.c_void_p), ("first_frame", C.c_longlong),
                ("n_frames", C.c_longlong), ("dst", C.c_void_p), ("dst_cap", C.c_size_t)]


class _LoudnessSpec(C.Structure):                  # include/pdmp3_bulk.h pdmp3_amd_loudness_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("n_samples", C.c_longlong), ("width", C.c_int), ("rolloff", C.c_double),
                ("target", C.c_double), ("peak_limit", C.c_double), ("dual_mono", C.c_int)]


def _loudness_spec(n_samples=0, sample_rate=0, channels=0, target=None, peak_limit=0.0, dual_mono=False, width=0, rolloff=0.0):
    return _LoudnessSpec(int(sample_rate), int(channels), int(n_samples), int(width), float(rolloff),
                         float("nan") if target is None else float(target), float(peak_limit), int(dual_mono))


def loudness_check(sample_rate, channels=1, **kw):
    """pdmp3_amd_loudness_check -> True when pdmp3_amd_bulk_decode_clips_loudness would accept these numbers (decode_clips_loudness's
    target, peak_limit, dual_mono) at sample_rate and `channels` channels"""
    return _check(_loudness_spec, "pdmp3_amd_loudness_check", sample_rate, dict(kw, channels=channels), (ValueError, OverflowError, TypeError), channels)


def loudness_coefficients(sample_rate):
    """pdmp3_amd_loudness_coefficients -> float64 [2, 2, 3]: [filter H1 / H2][b / a][3], the K-weighting's two biquads"""
    c = np.zeros(12, dtype=np.float64)
    if load_library().pdmp3_amd_loudness_coefficients(int(sample_rate), c.ctypes.data) != 0:
        raise ValueError("pdmp3_amd_loudness_coefficients: bad argument")
    return c.reshape(2, 2, 3)


def loudness_tables(sample_rate):
    """pdmp3_amd_loudness_tables -> (Hm float32 [64, 64], O float32 [64, 4], Phi float64 [4, 4], R float64 [4, 64], powers of Phi
    float64 [70, 4, 4]) as the loudness kernels read them"""
    hm, o = np.zeros((64, 64), dtype=np.float32), np.zeros((64, 4), dtype=np.float32)
    phi, r, pw = np.zeros((4, 4), dtype=np.float64), np.zeros((4, 64), dtype=np.float64), np.zeros((70, 4, 4), dtype=np.float64)
    if load_library().pdmp3_amd_loudness_tables(int(sample_rate), hm.ctypes.data, o.ctypes.data, phi.ctypes.data, r.ctypes.data, pw.ctypes.data) != 0:
        raise ValueError("pdmp3_amd_loudness_tables: bad argument")
    return hm, o, phi, r, pw


def loudness_plan(sample_rate, n_samples):
    """pdmp3_amd_loudness_plan -> (samples of a block, blocks of a scan chunk, LDS bytes of a workgroup of k_loud_blocks, q, chunks
    of a row, I, J)"""
    return _plan(load_library().pdmp3_amd_loudness_plan, (int(sample_rate), int(n_samples)), (_I, _I, _U, _I) + (_LL,) * 3)


class _R128Spec(C.Structure):                      # include/pdmp3_bulk.h pdmp3_amd_r128_spec
    _fields_ = [("loudness", _LoudnessSpec), ("limit_true_peak", C.c_int)]


def _r128_spec(n_samples=0, sample_rate=0, channels=0, target=None, peak_limit=0.0, limit_true_peak=True, dual_mono=False, width=0, rolloff=0.0):
    return _R128Spec(_loudness_spec(n_samples, sample_rate, channels, target, peak_limit, dual_mono, width, rolloff), int(limit_true_peak))


def r128_check(sample_rate, channels=1, **kw):
    """pdmp3_amd_r128_check -> True when pdmp3_amd_bulk_decode_clips_r128 would accept these numbers (decode_clips_r128's n_samples,
    target, peak_limit, limit_true_peak, dual_mono) at sample_rate and `channels` channels"""
    return _check(_r128_spec, "pdmp3_amd_r128_check", sample_rate, dict(kw, channels=channels), (ValueError, OverflowError, TypeError), channels)


def r128_taps():
    """pdmp3_amd_r128_taps -> (h float64 [49], the 4x interpolator; phases float32 [3, 12], c_p[d] = h[4 d + p] of p = 1 .. 3 as
    the kernel reads them)"""
    h, ph = np.zeros(49, dtype=np.float64), np.zeros((3, 12), dtype=np.float32)
    if load_library().pdmp3_amd_r128_taps(h.ctypes.data, ph.ctypes.data) != 0:
        raise ValueError("pdmp3_amd_r128_taps failed")
    return h, ph


def r128_plan(sample_rate, n_samples):
    """pdmp3_amd_r128_plan -> loudness_plan's seven numbers, then Js (3 s windows), Jr (those of the range) and Jsmax (floats of a
    row of short_term)"""
    return _plan(load_library().pdmp3_amd_r128_plan, (int(sample_rate), int(n_samples)), (_I, _I, _U, _I) + (_LL,) * 6)


class _PitchSpec(C.Structure):                     # include/pdmp3_bulk.h pdmp3_amd_pitch_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("width", C.c_int), ("rolloff", C.c_double), ("n_frames", C.c_longlong),
                ("frame_length", C.c_int), ("win_length", C.c_int), ("hop", C.c_int), ("fmin", C.c_double), ("fmax", C.c_double),
                ("threshold", C.c_double), ("out_mode", C.c_int)]


PITCH_MODES = {"pitch": 0, "curve": 1}
PITCH_FMIN, PITCH_FMAX = 65.406, 2093.0            # C2 and C7, librosa's note_to_hz to the digits its examples print


def _pitch_spec(n_frames=1, sample_rate=22050, frame_length=2048, win_length=None, hop=None, fmin=PITCH_FMIN, fmax=PITCH_FMAX, threshold=0.1,
                out_mode="pitch", channels=1, width=0, rolloff=0.0):
    """(None means 0 to the library: win_length frame_length / 2, hop frame_length / 4)"""
    return _PitchSpec(int(sample_rate), int(channels), int(width), float(rolloff), int(n_frames), int(frame_length),
                      0 if win_length is None else int(win_length), 0 if hop is None else int(hop), float(fmin), float(fmax), float(threshold),
                      _enum(PITCH_MODES, out_mode))


def pitch_check(sample_rate=22050, **kw):
    """pdmp3_amd_pitch_check -> True when pdmp3_amd_bulk_decode_clips_pitch would accept these numbers (decode_clips_pitch's
    argument names) at sample_rate"""
    return _check(_pitch_spec, "pdmp3_amd_pitch_check", sample_rate, kw, (ValueError, KeyError, OverflowError, TypeError))


def pitch_lags(sample_rate=22050, **kw):
    """pdmp3_amd_pitch_lags -> (tmin, tmax, lag tiles of 256 a frame)"""
    spec = _pitch_spec(sample_rate=sample_rate, **kw)
    return _plan(load_library().pdmp3_amd_pitch_lags, (C.byref(spec), int(sample_rate)), (_I, _I, _I))


def pitch_plan(sample_rate=22050, **kw):
    """pdmp3_amd_pitch_plan -> (frames of a workgroup of k_clip_pitch, LDS floats of its span, LDS bytes, matrix instructions a
    lag tile)"""
    spec = _pitch_spec(sample_rate=sample_rate, **kw)
    return _plan(load_library().pdmp3_amd_pitch_plan, (C.byref(spec), int(sample_rate)), (_I, _U, _U, _I))


class _PyinSpec(C.Structure):                      # include/pdmp3_bulk.h pdmp3_amd_pyin_spec
    _fields_ = [("pitch", _PitchSpec), ("n_thresholds", C.c_int), ("beta_a", C.c_double), ("beta_b", C.c_double),
                ("threshold_weights", C.c_void_p), ("boltzmann", C.c_double), ("resolution", C.c_double), ("max_transition_rate", C.c_double),
                ("switch_prob", C.c_double), ("no_trough_prob", C.c_double), ("fill", C.c_float), ("use_bin_frequency", C.c_int),
                ("out_mode", C.c_int)]


PYIN_MODES = {"pitch": 0, "observation": 1}


def _pyin_spec(n_frames=1, sample_rate=22050, channels=0, frame_length=2048, win_length=0, hop=0, fmin=PITCH_FMIN, fmax=PITCH_FMAX, n_thresholds=100,
               beta=(2, 18), threshold_weights=None, boltzmann=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01,
               no_trough_prob=0.01, fill=float("nan"), out_mode="pitch", width=0, rolloff=0.0):
    """-> (spec, what its threshold_weights points to).  fill None: the bin's frequency on unvoiced frames (librosa's
    fill_na=None); win_length / hop 0 or None: frame_length / 2, frame_length / 4"""
    pitch = _pitch_spec(n_frames, sample_rate, frame_length, win_length or None, hop or None, fmin, fmax, 0.1, 1, channels, width, rolloff)
    keep = None
    if threshold_weights is not None:
        keep = np.ascontiguousarray(threshold_weights, dtype=np.float64)
        if keep.shape != (int(n_thresholds),):
            raise ValueError("threshold_weights must hold n_thresholds values")
    a, b = beta
    spec = _PyinSpec(pitch, int(n_thresholds), float(a), float(b), None if keep is None else keep.ctypes.data, float(boltzmann), float(resolution),
                     float(max_transition_rate), float(switch_prob), float(no_trough_prob), 0.0 if fill is None else float(fill),
                     1 if fill is None else 0, _enum(PYIN_MODES, out_mode))
    return spec, keep


def pyin_check(sample_rate=22050, **kw):
    """pdmp3_amd_pyin_check -> True when pdmp3_amd_bulk_decode_clips_pyin would accept these numbers (decode_clips_pyin's
    argument names) at sample_rate"""
    return _check(_pyin_spec, "pdmp3_amd_pyin_check", sample_rate, kw, (ValueError, KeyError, OverflowError, TypeError))


def pyin_tables(sample_rate=22050, **kw):
    """pdmp3_amd_pyin_tables -> dict of every table the kernels read: theta, w, wsum, G, cN, T, ltri (offsets -hb .. hb), lZ as
    float64 numpy, f0 (the bins' frequencies) as float32, the scalars l_stay, l_sw, L0, lp0_u, the kernels' block, and the counts n_thresholds, max_troughs, n_bins, hb"""
    spec, keep = _pyin_spec(sample_rate=sample_rate, **kw)
    lib = load_library()
    counts = (C.c_int * 4)()
    n = lib.pdmp3_amd_pyin_tables(C.byref(spec), int(sample_rate), None, 0, counts)
    if n < 0:
        raise ValueError("pdmp3_amd_pyin_tables: bad argument")
    t = np.zeros(n, dtype=np.float64)
    if lib.pdmp3_amd_pyin_tables(C.byref(spec), int(sample_rate), t.ctypes.data_as(C.c_void_p), t.size, counts) != n:
        raise ValueError("pdmp3_amd_pyin_tables: bad argument")
    nt, mt, nb, hb = (int(x) for x in counts)
    out, at = dict(n_thresholds=nt, max_troughs=mt, n_bins=nb, hb=hb, block=t), 0
    for name, size in (("theta", nt), ("w", nt), ("wsum", nt + 1), ("G", mt), ("cN", mt + 1), ("T", nb), ("ltri", 2 * hb + 1), ("lZ", nb)):
        out[name] = t[at:at + size].copy()
        at += size
    out["f0"] = t[at:].view(np.float32)[:nb].copy()
    out["l_stay"], out["l_sw"], out["L0"], out["lp0_u"] = (float(x) for x in t[-4:])
    out["block"] = t[:-4]
    return out


def pyin_plan(sample_rate=22050, **kw):
    """pdmp3_amd_pyin_plan -> dict: states, n_bins, n_s, msf, band (Wd), hb, obs_frames (waves of a workgroup of k_clip_pyin_obs),
    path_threads, obs_lds, path_lds (bytes), and the stage bytes of a (clip, channel): curve_bytes, obs_bytes, bp_bytes"""
    spec, keep = _pyin_spec(sample_rate=sample_rate, **kw)
    v, lds, st = (C.c_int * 8)(), (C.c_uint * 2)(), (C.c_ulonglong * 3)()
    if load_library().pdmp3_amd_pyin_plan(C.byref(spec), int(sample_rate), v, lds, st) != 0:
        raise ValueError("pdmp3_amd_pyin_plan: bad argument")
    names = ("states", "n_bins", "n_s", "msf", "band", "hb", "obs_frames", "path_threads")
    return dict(zip(names, (int(x) for x in v)), obs_lds=int(lds[0]), path_lds=int(lds[1]), curve_bytes=int(st[0]), obs_bytes=int(st[1]),
                bp_bytes=int(st[2]))


class _TempogramSpec(C.Structure):                 # include/pdmp3_bulk.h pdmp3_amd_tempogram_spec
    _fields_ = [("mel", _MelLongSpec), ("lag", C.c_int), ("max_size", C.c_int), ("win_length", C.c_int), ("start_bpm", C.c_double),
                ("std_bpm", C.c_double), ("max_tempo", C.c_double), ("out_mode", C.c_int)]


TEMPOGRAM_MODES = {"onset": 0, "tempogram": 1, "tempo": 2}


def _tempogram_spec(n_frames=1, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, lag=1, max_size=1, win_length=384, start_bpm=120.0,
                    std_bpm=1.0, max_tempo=320.0, out_mode="tempogram", f_min=0.0, f_max=0.0, scale="slaney", norm="slaney", floor=1e-10,
                    fft_win_length=None, fft_window=None, channels=1, width=0, rolloff=0.0):
    """-> (spec, what its window points to).  win_length is the tempogram's; the transform's window is fft_win_length /
    fft_window (decode_clips_mel_long's win_length / window)"""
    mel, keep = _mel_long_spec(n_frames, sample_rate, n_fft, hop, n_mels, f_min, f_max, scale, norm, "log10", floor, fft_win_length, fft_window,
                               channels, width, rolloff)
    return _TempogramSpec(mel, int(lag), int(max_size), int(win_length), float(start_bpm), float(std_bpm), float(max_tempo),
                          _enum(TEMPOGRAM_MODES, out_mode)), keep


def tempogram_check(sample_rate=22050, **kw):
    """pdmp3_amd_tempogram_check -> True when pdmp3_amd_bulk_decode_clips_tempogram would accept these numbers
    (decode_clips_tempogram's argument names) at sample_rate"""
    return _check(_tempogram_spec, "pdmp3_amd_tempogram_check", sample_rate, kw, (ValueError, KeyError, OverflowError, TypeError))


def tempogram_window(win_length=384):
    """pdmp3_amd_tempogram_window -> float32 numpy [win_length]: the periodic Hann window k_clip_tempogram reads"""
    w = np.full(max(int(win_length), 1), np.nan, dtype=np.float32)
    if load_library().pdmp3_amd_tempogram_window(int(win_length), w.ctypes.data_as(C.c_void_p), w.size) != int(win_length):
        raise ValueError("pdmp3_amd_tempogram_window: win_length must be even, 16 .. 1024")
    return w


def tempogram_prior(sample_rate=22050, **kw):
    """pdmp3_amd_tempogram_prior -> (float64 numpy [win_length]: the log-normal prior of every lag, -inf where a lag is not
    admissible; the smallest admissible lag)"""
    spec, keep = _tempogram_spec(sample_rate=sample_rate, **kw)
    p = np.full(max(spec.win_length, 1), np.nan, dtype=np.float64)
    first = C.c_int(0)
    if load_library().pdmp3_amd_tempogram_prior(C.byref(spec), int(sample_rate), p.ctypes.data_as(C.c_void_p), p.size, C.byref(first)) != 0:
        raise ValueError("pdmp3_amd_tempogram_prior: bad argument")
    return p, first.value


def tempogram_plan(sample_rate=22050, **kw):
    """pdmp3_amd_tempogram_plan -> (log-mel frames in front of frame 0, behind the last frame, lag tiles of 256, matrix
    instructions a lag tile, frames of a workgroup of k_clip_tempogram, its LDS bytes)"""
    spec, keep = _tempogram_spec(sample_rate=sample_rate, **kw)
    return _plan(load_library().pdmp3_amd_tempogram_plan, (C.byref(spec), int(sample_rate)), (_I,) * 5 + (_U,))


class _BeatSpec(C.Structure):                      # include/pdmp3_bulk.h pdmp3_amd_beat_spec
    _fields_ = [("tg", _TempogramSpec), ("bpm", C.c_double), ("tightness", C.c_double), ("trim", C.c_int), ("out_mode", C.c_int)]


BEAT_MODES = {"score": 0, "dp": 1, "beats": 2}
BEAT_STATS = ("bpm", "period", "kept", "beats", "tail", "norm", "threshold", "frames")


def _beat_spec(n_frames=1, sample_rate=22050, bpm=0.0, tightness=100.0, trim=True, out_mode="beats", **kw):
    """-> (spec, what its window points to).  kw: decode_clips_tempogram's arguments without out_mode"""
    tg, keep = _tempogram_spec(n_frames, sample_rate, out_mode="onset", **kw)
    return _BeatSpec(tg, float(bpm), float(tightness), 1 if trim else 0, _enum(BEAT_MODES, out_mode)), keep


def beat_check(sample_rate=22050, **kw):
    """pdmp3_amd_beat_check -> True when pdmp3_amd_bulk_decode_clips_beats would accept these numbers (decode_clips_beats's
    argument names) at sample_rate"""
    return _check(_beat_spec, "pdmp3_amd_beat_check", sample_rate, kw, (ValueError, KeyError, OverflowError, TypeError))


def beat_tables(period, sample_rate=22050, **kw):
    """pdmp3_amd_beat_tables -> (g float64 [period + 1], tx float64 [2 period + 1]) as the kernels read them for this period: the
    local score's Gaussian taps and the programme's transition cost (its entries below h are 0 and not read)"""
    spec, keep = _beat_spec(sample_rate=sample_rate, **kw)
    p = int(period)
    g, tx = np.full(max(p, 0) + 1, np.nan), np.full(2 * max(p, 0) + 1, np.nan)
    if load_library().pdmp3_amd_beat_tables(C.byref(spec), int(sample_rate), p, g.ctypes.data_as(C.c_void_p), tx.ctypes.data_as(C.c_void_p)) != 0:
        raise ValueError("pdmp3_amd_beat_tables: bad argument")
    return g, tx


def beat_plan(sample_rate=22050, **kw):
    """pdmp3_amd_beat_plan -> dict: period (0: estimated), h, p_min, p_max (the periods the tables hold), threads, steps (of the
    programme), lanes (of a frame), frames (of a pass of a step), score_lds, dp_lds (bytes), work_bytes (the scratch of a clip and
    channel), table_bytes"""
    spec, keep = _beat_spec(sample_rate=sample_rate, **kw)
    v, lds, st = (C.c_int * 8)(), (C.c_uint * 2)(), (C.c_ulonglong * 2)()
    if load_library().pdmp3_amd_beat_plan(C.byref(spec), int(sample_rate), v, lds, st) != 0:
        raise ValueError("pdmp3_amd_beat_plan: bad argument")
    names = ("period", "h", "p_min", "p_max", "threads", "steps", "lanes", "frames")
    return dict(zip(names, (int(x) for x in v)), score_lds=int(lds[0]), dp_lds=int(lds[1]), work_bytes=int(st[0]), table_bytes=int(st[1]))


class _AudioClip(C.Structure):                     # include/pdmp3_bulk.h pdmp3_amd_audio_clip
    _fields_ = [("mp3", C.c_void_p), ("n", C.c_size_t), ("index", C.c_void_p), ("start", C.c_longlong), ("dst", C.c_void_p),
                ("chan_stride", C.c_size_t)]


class _AudioSpec(C.Structure):                     # include/pdmp3_bulk.h pdmp3_amd_audio_spec
    _fields_ = [("rate", C.c_long), ("channels", C.c_int), ("n_samples", C.c_longlong), ("width", C.c_int), ("rolloff", C.c_double)]


def _clip_destination(out, k, c, inner, complex_ok=False):
    """Where the rows of a clip call go: `out` -- a torch tensor or a numpy array -- seen as float32 [>= k, c] + inner (complex64
    where complex_ok: as [..., 2], inner's last dimension) -> (address of row 0, bytes between rows, floats between channels).
    Rows and channels may be strided, a channel's floats not; AssertionError for anything else."""
    if hasattr(out, "data_ptr"):
        import torch
        v = torch.view_as_real(out) if out.is_complex() else out
        assert v.dtype == torch.float32 and (complex_ok or not out.is_complex())
        shape, strides, base = tuple(v.shape), tuple(v.stride()), v.data_ptr()
    else:
        v = out.view(np.float32).reshape(out.shape + (2,)) if out.dtype == np.complex64 else out
        assert v.dtype == np.float32 and (complex_ok or out.dtype != np.complex64) and all(s % 4 == 0 for s in v.strides)
        shape, strides, base = v.shape, tuple(s // 4 for s in v.strides), v.ctypes.data
    inner = tuple(inner)
    assert len(shape) == 2 + len(inner) and shape[1:] == (c,) + inner and shape[0] >= k
    want = 1
    for n, s in zip(reversed(inner), reversed(strides[2:])):                       # (a row's floats are dense)
        assert n <= 1 or s == want or 0 in shape               # (an array without elements has strides of no meaning)
        want *= n
    return base, strides[0] * 4, strides[1]


def _address(a):
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


def _stats_like(out, shape):
    """float32 `shape` full of NaN where a clip call's stats go: a torch tensor on out's device (the current one without out),
    or a numpy array where out is one"""
    if out is None or hasattr(out, "data_ptr"):
        import torch
        stats = torch.full(shape, float("nan"), dtype=torch.float32, device=torch.device("cuda", torch.cuda.current_device()) if out is None else out.device)
        torch.cuda.synchronize()
        return stats
    return np.full(shape, np.nan, dtype=np.float32)


def _aux_destination(name, dst, k, want_cols, cols="n"):
    """an auxiliary destination of a loudness call, float32 [>= k, want_cols()], contiguous, torch or numpy -> its address;
    want_cols() None: any width (the library refuses the call, or writes nothing)"""
    ok = (dst.is_contiguous() and str(dst.dtype) == "torch.float32") if hasattr(dst, "data_ptr") else (dst.flags["C_CONTIGUOUS"] and dst.dtype == np.float32)
    assert ok and len(dst.shape) == 2 and dst.shape[0] >= k, "%s: float32 [>= K, %s], contiguous" % (name, cols)
    n = want_cols()
    assert n is None or dst.shape[1] == n, "%s: float32 [>= K, %s]" % (name, n)
    return _address(dst)


def _plan_field(call, plan, field, clips, sample_rate, n_samples):
    """plan(rate, n_samples)[field] at the rate of decode_clips_<call>: sample_rate, or the clips' own where they share one; None
    without a rate or samples"""
    rates = set(ix.rate for _, ix, _ in clips if not ix.replay and ix.one_format and ix.frames)
    fs = int(sample_rate) or (rates.pop() if len(rates) == 1 else 0)
    if not (fs and n_samples):
        return None
    try:
        return plan(fs, n_samples)[field]
    except ValueError:
        raise RuntimeError("pdmp3_amd_bulk_decode_clips_%s: bad sample_rate or n_samples" % call)


class BulkDecoder:
    """include/pdmp3_bulk.h: whole-stream decode, host Huffman on a thread pool + pipelined GPU batches.
    parse_only=True: host stages only (records out), for machines without a GPU."""

    def __init__(self, threads=0, window_frames=0, parse_only=False, host_huffman=False, device=None):
        """host_huffman=False: scalefactors + Huffman run on the device (pdmp3_hip_stream_submit_bits), the pool only
        copies PCM out; True: they run on the pool's threads (the engine gets decoded records)."""
        self.lib = load_library()
        self.parse_only = parse_only
        if parse_only:
            self.h = self.lib.pdmp3_amd_bulk_new_parse_only(threads, window_frames)
        elif device is not None:
            self.h = self.lib.pdmp3_amd_bulk_new_on(threads, window_frames, 1 if host_huffman else 0, int(device))
        else:
            self.h = self.lib.pdmp3_amd_bulk_new_ex(threads, window_frames, 1 if host_huffman else 0)
        if not self.h:
            raise RuntimeError("pdmp3_amd_bulk_new failed (no MI355X transform engine; there is no CPU fallback)")
        self.threads = self.lib.pdmp3_amd_bulk_threads(self.h)

    def close(self):
        if self.h:
            self.lib.pdmp3_amd_bulk_delete(self.h)
            self.h = None

    def set_quirks(self, iso_mask):
        self.lib.pdmp3_amd_bulk_set_quirks.argtypes = [C.c_void_p, C.c_uint]
        if self.lib.pdmp3_amd_bulk_set_quirks(self.h, iso_mask) != 0:
            raise ValueError("pdmp3_amd_bulk_set_quirks: unknown bits in %#x" % iso_mask)
        self.iso = iso_mask

    def decode_into(self, mp3, out: np.ndarray):
        a = _as_u8(mp3)
        rate, ch = C.c_long(0), C.c_int(0)
        total = self.lib.pdmp3_amd_bulk_decode(self.h, a.ctypes.data_as(C.c_void_p), len(mp3),
                                               out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(rate), C.byref(ch))
        if total == -2:
            raise RingReplay("the reference replays its input ring on this stream (no finite output)")
        if total < 0:
            raise RuntimeError("pdmp3_amd_bulk_decode: engine failure")
        return total, rate.value, ch.value

    def decode_into_async(self, mp3, out: np.ndarray):
        """queue one stream; `out` is complete after wait()"""
        a = _as_u8(mp3)
        rate, ch = C.c_long(0), C.c_int(0)
        total = self.lib.pdmp3_amd_bulk_decode_async(self.h, a.ctypes.data_as(C.c_void_p), len(mp3),
                                                     out.ctypes.data_as(C.c_void_p), out.nbytes, C.byref(rate), C.byref(ch))
        if total == -2:
            raise RingReplay("the reference replays its input ring on this stream (no finite output)")
        if total < 0:
            raise RuntimeError("pdmp3_amd_bulk_decode_async: engine failure")
        return total, rate.value, ch.value

    def decode_into_device(self, mp3, out_tensor, wait=True):
        """PCM into a torch int16 tensor on the GPU.  Windows of one channel count go from the engine's buffer to the
        tensor without leaving the device; a window that mixes mono and stereo frames, or the one the tensor ends in,
        is staged in pinned host memory and copied from there.  The decoder writes from its own HIP streams, which do not
        wait for torch's: work of the caller's that is still pending on the tensor (a fill, say) must be through first
        (torch.cuda.synchronize()), and with wait=False the tensor is the decoder's until wait() has returned."""
        a = _as_u8(mp3)
        rate, ch = C.c_long(0), C.c_int(0)
        f = self.lib.pdmp3_amd_bulk_decode if wait else self.lib.pdmp3_amd_bulk_decode_async
        total = f(self.h, a.ctypes.data_as(C.c_void_p), len(mp3), C.c_void_p(out_tensor.data_ptr()),
                  out_tensor.numel() * out_tensor.element_size(), C.byref(rate), C.byref(ch))
        if total == -2:
            raise RingReplay("the reference replays its input ring on this stream (no finite output)")
        if total < 0:
            raise RuntimeError("pdmp3_amd_bulk_decode: engine failure")
        return total, rate.value, ch.value

    def split_scans(self):
        """-> (streams the split scan decoded to their end, streams it gave up half way and handed to the one-thread scan)"""
        a, g = C.c_longlong(0), C.c_longlong(0)
        self.lib.pdmp3_amd_bulk_split_scans(self.h, C.byref(a), C.byref(g))
        return a.value, g.value

    def huffman_frames(self):
        """-> (frames whose scalefactors + Huffman data the device decoded, frames the host pool decoded), over the
        decoder's life"""
        d, h = C.c_longlong(0), C.c_longlong(0)
        self.lib.pdmp3_amd_bulk_huffman_frames(self.h, C.byref(d), C.byref(h))
        return d.value, h.value

    def wait(self):
        if self.lib.pdmp3_amd_bulk_wait(self.h) != 0:
            raise RuntimeError("pdmp3_amd_bulk_wait: engine failure")

    def decode_many(self, mp3s):
        """-> list of int16 PCM arrays, one per stream, each exactly the CLI driver's output for its bytes; the
        streams go through the pipeline back to back (pdmp3_amd_bulk_decode_async)."""
        outs = []
        for m in mp3s:
            total, _ = scan_buffer(m, getattr(self, "iso", 0))
            out = np.empty(max(total, 2) // 2, dtype=np.int16)
            got, _, _ = self.decode_into_async(m, out)
            assert got == total, (got, total)
            outs.append(out[:total // 2])
        self.wait()
        return outs

    def decode(self, mp3):
        """-> interleaved int16 PCM (numpy), exactly the CLI driver's output for these bytes."""
        total, _ = scan_buffer(mp3, getattr(self, "iso", 0))
        out = np.empty(max(total, 2) // 2, dtype=np.int16)
        got, rate, ch = self.decode_into(mp3, out)
        assert got == total, (got, total)
        return out[:total // 2]

    def decode_clips(self, clips, out):
        """pdmp3_amd_bulk_decode_clips: clips = sequence of (mp3, StreamIndex, first frame, frames); out = ONE int16 array
        of shape [K, stride] -- a torch tensor (device memory of the decoder's GPU, or host memory) or a numpy array
        (pageable, or a view of pinned memory) -- or a list of K contiguous 1-D ones; row k receives clip k's PCM: exactly the bytes [pcm_offsets[a],
        pcm_offsets[b]) of the whole-stream output for the clip's clamped range [a, b), as far as the row holds them.  Bytes
        past a clip's count are not written.  Synchronous.  -> numpy int64 byte counts, one per clip.  RingReplay (with
        .pcm_bytes) when a clip's stream is one the scan calls a ring replay; the other clips are decoded all the same."""
        k = len(clips)
        if isinstance(out, (list, tuple)):             # (or one 1-D int16 buffer per clip)
            assert len(out) >= k
            dst = [_int16_buffer(o, 1) for o in out[:k]]
        elif hasattr(out, "data_ptr"):
            assert out.dim() == 2 and out.shape[0] >= k and out.stride(1) == 1 and out.element_size() == 2
            dst = [(out.data_ptr() + i * out.stride(0) * 2, out.shape[1] * 2) for i in range(k)]
        else:
            assert out.ndim == 2 and out.shape[0] >= k and out.strides[1] == 2 and out.dtype == np.int16
            dst = [(out.ctypes.data + i * out.strides[0], out.shape[1] * 2) for i in range(k)]
        arr = (_Clip * max(k, 1))()
        keep = []
        for i, (mp3, ix, first, count) in enumerate(clips):
            a = _as_u8(mp3)
            keep.append(a)
            arr[i] = _Clip(a.ctypes.data, len(mp3), ix.h, int(first), int(count), dst[i][0], dst[i][1])
        got = (C.c_longlong * max(k, 1))()
        rc = self.lib.pdmp3_amd_bulk_decode_clips(self.h, arr, k, got)
        pcm_bytes = np.array(got[:k], dtype=np.int64)
        if rc == PDMP3_BULK_REPLAY:
            e = RingReplay("the reference replays its input ring on a clip's stream (no finite output)")
            e.pcm_bytes = pcm_bytes
            raise e
        if rc != 0:
            raise RuntimeError("pdmp3_amd_bulk_decode_clips failed (a bad argument, a decoder without device Huffman, switches "
                               "that differ from an index's, or an engine failure)")
        return pcm_bytes

    def decode_range(self, mp3, index, first, count):
        """frames [first, first + count) of the stream (clamped to index.frames) -> int16 numpy: exactly that slice of
        decode(mp3)"""
        if index.replay:
            raise RingReplay("the reference replays its input ring on this stream (no finite output)")
        a, b = index.clamp(first, count)
        nbytes = int(index.pcm_offsets[b] - index.pcm_offsets[a])
        out = np.empty((1, max(nbytes // 2, 1)), dtype=np.int16)
        got = self.decode_clips([(mp3, index, first, count)], out)
        assert got[0] == nbytes, (got[0], nbytes)
        return out[0, :nbytes // 2]

    def decode_clips_audio(self, clips, n_samples, sample_rate=0, channels=0, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_audio: clips = sequence of (mp3, StreamIndex, first sample at the new rate) -> (out, valid):
        out float32 [K, C, n_samples], planar, every clip at sample_rate (0: each stream's own) with `channels` channels (0: the
        clips' common count), resampled on the GPU by a Hann-windowed sinc (width zero crossings, default 6; rolloff, default
        0.99: torchaudio's sinc_interp_hann), zeros behind a stream's end; valid[k] = samples of row k that lie inside the
        stream.  out: a float32 torch tensor on the decoder's device (made when not given; its rows and channels may be
        strided, the samples not) or a numpy array.  Synchronous.  RingReplay / MixedFormat (with .out and .valid: those
        clips' rows are not written, valid is PDMP3_BULK_REPLAY / PDMP3_BULK_MIXED_FORMAT there) when a clip's stream has no
        finite output / no one format; the other clips are decoded all the same."""
        t = int(n_samples)
        return self._clips_call("audio", clips, (t,), lambda: (_AudioSpec(int(sample_rate), int(channels), t, int(width), float(rolloff)), None), channels, out)

    def decode_clips_mel(self, clips, n_frames, sample_rate=16000, n_fft=400, hop=160, n_mels=80, f_min=0.0, f_max=0.0, scale="slaney",
                         norm="slaney", mode="log10", floor=1e-10, channels=1, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_mel: clips = sequence of (mp3, StreamIndex, first sample at sample_rate) -> (out, valid):
        out float32 [K, C, n_mels, n_frames], frame f of a clip centred on sample start + f hop of the stream resampled as
        decode_clips_audio does (width, rolloff), periodic Hann window of n_fft, zeros outside the stream and no reflection;
        scale "slaney" / "htk", norm "slaney" / None, mode "power" / "log" / "log10" / "whisper", floor the clamp of the log modes;
        valid[k] = frames of row k whose centre lies inside the stream.  out: a float32 torch tensor on the decoder's device (made
        when not given; rows and channels may be strided) or a numpy array.  Synchronous.  RingReplay / MixedFormat (with .out
        and .valid) as decode_clips_audio."""
        f, nm = int(n_frames), int(n_mels)
        spec = lambda: (_mel_spec(f, sample_rate, n_fft, hop, nm, f_min, f_max, scale, norm, mode, floor, channels, width, rolloff), None)
        return self._clips_call("mel", clips, (nm, f), spec, channels, out)

    def decode_clips_mel_long(self, clips, n_frames, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, f_min=0.0, f_max=0.0, scale="slaney",
                              norm="slaney", mode="log10", floor=1e-10, win_length=None, window=None, channels=1, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_mel_long: decode_clips_mel in everything -- clips, framing, filterbank, out, valid,
        exceptions -- at n_fft 2048 or 4096, with decode_clips_stft_long's win_length / window (periodic Hann of win_length when
        no window is given); mode "power" / "log" / "log10" ("whisper" is refused).  The transform, the powers and the
        filterbank run in one kernel, k_clip_mel_long: no spectrum is written."""
        f, nm = int(n_frames), int(n_mels)
        spec = lambda: _mel_long_spec(f, sample_rate, n_fft, hop, nm, f_min, f_max, scale, norm, mode, floor, win_length, window, channels, width, rolloff)
        return self._clips_call("mel_long", clips, (nm, f), spec, channels, out)

    def decode_clips_spectral(self, clips, n_frames, sample_rate=22050, n_fft=2048, hop=512, roll_percent=0.85, amin=1e-10, zcr_threshold=1e-10,
                              channels=0, win_length=None, window=None, out=None, width=0, rolloff=0.0):
        """pdmp3_amd_bulk_decode_clips_spectral: clips as decode_clips_stft_long takes them -> (out, valid): out float32
        [K, C, 6, n_frames], the rows SPECTRAL_ROWS -- librosa.feature's rms (frame_length = n_fft), zero_crossing_rate
        (threshold = zcr_threshold, pad = False), spectral_centroid, spectral_bandwidth (p = 2), spectral_rolloff (roll_percent) and
        spectral_flatness (amin, power = 2) -- of frame f centred on sample start + f hop, the stream's own neighbours around the
        clip, zeros outside the stream and no reflection.  n_fft 2048 or 4096; win_length / window as decode_clips_stft_long.
        One kernel, k_clip_spectral: no spectrum is written.  valid, out, the exceptions: as decode_clips_mel_long."""
        f = int(n_frames)
        spec = lambda: _spectral_spec(f, sample_rate, n_fft, hop, roll_percent, amin, zcr_threshold, channels, win_length, window, width, rolloff)
        return self._clips_call("spectral", clips, (len(SPECTRAL_ROWS), f), spec, channels, out, refused=(ValueError, OverflowError, TypeError))

    def decode_clips_hpss(self, clips, n_frames, sample_rate=22050, n_fft=2048, hop=512, kernel_size=31, power=2.0, margin=1.0, mode="mask",
                          channels=0, win_length=None, window=None, out=None, width=0, rolloff=0.0):
        """pdmp3_amd_bulk_decode_clips_hpss: clips as decode_clips_stft_long takes them -> (out, valid): median-filter
        harmonic-percussive separation (librosa.decompose.hpss) of the magnitudes decode_clips_stft_long gives for frame f centred
        on sample start + f hop.  out[:, :, 0] is the harmonic component, out[:, :, 1] the percussive one; mode "mask": float32
        [K, C, 2, n_fft / 2 + 1, n_frames], the soft masks (power 1, 2 or inf; margin >= 1); "magnitude": the masked magnitudes;
        "complex": complex64 of the same shape, the masked spectrum, which torch.istft takes; "median": the two median-filtered
        spectrograms.  kernel_size and margin: one number or (harmonic, percussive); sizes odd, 3 .. 31.  The harmonic median
        runs over the stream's own frames in front of and behind the clip (zeros outside the stream, no reflection along time),
        the percussive one reflects at bins 0 and n_fft / 2 as scipy's "reflect" does.  n_fft 2048 or 4096; win_length / window
        as decode_clips_stft_long.  valid, out, the exceptions: as decode_clips_mel_long."""
        f, nb = int(n_frames), int(n_fft) // 2 + 1
        m = HPSS_MODES.get(mode) if isinstance(mode, str) else mode
        if m not in (0, 1, 2, 3):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_hpss: mode is \"mask\", \"magnitude\", \"complex\" or \"median\"")
        spec = lambda: _hpss_spec(f, sample_rate, n_fft, hop, kernel_size, power, margin, m, channels, win_length, window, width, rolloff)
        return self._clips_call("hpss", clips, (2, nb, f, 2) if m == 2 else (2, nb, f), spec, channels, out, complex_ok=m == 2,
                                refused=(ValueError, OverflowError, TypeError))

    def decode_clips_mfcc_long(self, clips, n_frames, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, n_mfcc=20, lifter=0.0, top_db=80.0,
                               amin=1e-10, deltas=0, delta_width=9, out_mode="mfcc", out=None, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney",
                               win_length=None, window=None, channels=1, width=0, rolloff=0.0):
        """pdmp3_amd_bulk_decode_clips_mfcc_long: clips as decode_clips_mel_long takes them -> (out, valid).  out_mode "mfcc":
        float32 [K, C, (1 + deltas) n_mfcc, n_frames] -- librosa.feature.mfcc (orthonormal DCT-II of
        power_to_db(melspectrogram, ref=1.0, amin, top_db), lifter) of frame f centred on sample start + f hop, with deltas = 1 or 2
        librosa.feature.delta(width=delta_width) of order 1 and 2 stacked under it, as np.concatenate([mfcc, delta, delta2],
        axis=-2); the deltas read the stream's own frames in front of and behind the clip (zeros outside the stream), so the
        interior formula holds at every frame and there is no mode="interp" edge.  "db": [K, C, n_mels, n_frames], the dB mel
        itself.  top_db clamps at the largest value of the clip's own frames, per clip and channel (librosa takes one maximum
        over a stereo clip's channels); None: no clamp.  n_fft 2048 or 4096; the filterbank's and the window's arguments, valid,
        out, the exceptions: as decode_clips_mel_long."""
        f, nm, nc, nd = int(n_frames), int(n_mels), int(n_mfcc), int(deltas)
        m = MFCC_LONG_MODES.get(out_mode) if isinstance(out_mode, str) else out_mode
        if m not in (0, 1):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_mfcc_long: out_mode is \"mfcc\" or \"db\"")
        spec = lambda: _mfcc_long_spec(f, sample_rate, n_fft, hop, nm, n_mfcc, lifter, top_db, amin, deltas, delta_width, m, f_min, f_max, scale, norm,
                                       win_length, window, channels, width, rolloff)
        inner = (nm, f) if m == 1 else ((1 + nd) * nc, f)
        if nm < 1 or (m == 0 and (nd not in (0, 1, 2) or nc < 1)):        # (no shape to check a destination against)
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_mfcc_long: bad n_mels, n_mfcc or deltas")
        return self._clips_call("mfcc_long", clips, inner, spec, channels, out, refused=(ValueError, KeyError, OverflowError, TypeError))

    def decode_clips_fbank(self, clips, n_frames, sample_rate=16000, frame_length=25.0, frame_shift=10.0, num_mel_bins=23, win_length=None,
                           hop=None, round_to_power_of_two=True, remove_dc_offset=True, preemphasis_coefficient=0.97, window_type="povey",
                           blackman_coeff=0.42, low_freq=20.0, high_freq=0.0, use_log_fbank=True, use_energy=False, htk_compat=False,
                           energy_floor=1.0, subtract_mean=False, scale=1.0, channels=1, width=0, rolloff=0.0, out=None, **not_offered):
        """pdmp3_amd_bulk_decode_clips_fbank: clips = sequence of (mp3, StreamIndex, first sample at sample_rate) -> (out, valid):
        out float32 [K, C, n_frames, D], D = num_mel_bins + use_energy, what torchaudio.compliance.kaldi.fbank (its argument names
        and defaults) gives for scale * the stream resampled as decode_clips_audio does, frame f from sample start + f hop on,
        zeros outside the stream and no reflection; scale 32768.0: Kaldi's int16 convention.  win_length / hop in samples override
        frame_length / frame_shift in milliseconds.  valid[k] = frames of row k that lie wholly inside the stream (subtract_mean
        averages over them).  dither, use_power=False, raw_energy=False, snip_edges=False and vtln_warp are refused.  out: a
        float32 torch tensor on the decoder's device (made when not given; rows and channels may be strided) or a numpy array.
        Synchronous.  RingReplay / MixedFormat (with .out and .valid) as decode_clips_audio."""
        f, d = int(n_frames), int(num_mel_bins) + int(bool(use_energy))
        spec = lambda: (_fbank_spec(f, sample_rate, frame_length, frame_shift, num_mel_bins, win_length, hop, round_to_power_of_two, remove_dc_offset,
                                   preemphasis_coefficient, window_type, blackman_coeff, low_freq, high_freq, use_log_fbank, use_energy, htk_compat,
                                   energy_floor, subtract_mean, scale, channels, width, rolloff, **not_offered), None)
        return self._clips_call("fbank", clips, (f, d), spec, channels, out)

    def decode_clips_mfcc(self, clips, n_frames, sample_rate=16000, num_ceps=13, cepstral_lifter=22.0, num_mel_bins=23, frame_length=25.0,
                          frame_shift=10.0, win_length=None, hop=None, round_to_power_of_two=True, remove_dc_offset=True,
                          preemphasis_coefficient=0.97, window_type="povey", blackman_coeff=0.42, low_freq=20.0, high_freq=0.0, use_energy=False,
                          htk_compat=False, energy_floor=1.0, subtract_mean=False, scale=1.0, channels=1, width=0, rolloff=0.0, out=None,
                          **not_offered):
        """pdmp3_amd_bulk_decode_clips_mfcc: clips = sequence of (mp3, StreamIndex, first sample at sample_rate) -> (out, valid):
        out float32 [K, C, n_frames, num_ceps], what torchaudio.compliance.kaldi.mfcc (its argument names and defaults) gives for
        scale * the stream resampled as decode_clips_audio does: the cepstra of decode_clips_fbank's log filterbank, liftered, with
        C0 or (use_energy) the log energy in its place, in front or (htk_compat) behind the others.  Everything else --
        framing, valid, what is refused, `out`, RingReplay / MixedFormat -- as decode_clips_fbank.  Synchronous."""
        f, d = int(n_frames), int(num_ceps)
        spec = lambda: (_mfcc_spec(num_ceps, cepstral_lifter, n_frames=f, sample_rate=sample_rate, frame_length=frame_length, frame_shift=frame_shift,
                                  num_mel_bins=num_mel_bins, win_length=win_length, hop=hop, round_to_power_of_two=round_to_power_of_two,
                                  remove_dc_offset=remove_dc_offset, preemphasis_coefficient=preemphasis_coefficient, window_type=window_type,
                                  blackman_coeff=blackman_coeff, low_freq=low_freq, high_freq=high_freq, use_energy=use_energy,
                                  htk_compat=htk_compat, energy_floor=energy_floor, subtract_mean=subtract_mean, scale=scale, channels=channels,
                                  width=width, rolloff=rolloff, **not_offered), None)
        return self._clips_call("mfcc", clips, (f, d), spec, channels, out, made=(f, max(d, 0)))

    def decode_clips_stft(self, clips, n_frames, sample_rate=16000, n_fft=400, hop=160, win_length=None, window=None, normalized=False,
                          mode="complex", floor=1e-10, channels=1, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_stft: clips = sequence of (mp3, StreamIndex, first sample at sample_rate) -> (out, valid):
        the short-time Fourier transform [K, C, n_fft // 2 + 1, n_frames], frame f of a clip centred on sample start + f hop of the
        stream resampled as decode_clips_audio does (width, rolloff), zeros outside the stream and no reflection: torch.stft with
        center=False on the span from start - n_fft // 2 on.  window: win_length values (numpy or torch), None: the periodic
        Hann window of win_length (None: n_fft), centred in n_fft as torch.stft does; normalized: scaled by n_fft ** -0.5.
        mode "complex" (complex64) / "magnitude" / "power" / "log" / "log10" (float32; floor clamps the power of the last
        two).  valid[k] = frames of row k whose centre lies inside the stream.  out: a torch tensor on the decoder's device
        (made when not given; rows and channels may be strided) or a numpy array; mode "complex": complex64 [K, C, bins, F]
        or float32 [K, C, bins, F, 2].  Synchronous.  RingReplay / MixedFormat (with .out and .valid) as decode_clips_audio."""
        return self._clips_stft("stft", clips, n_frames, sample_rate, n_fft, hop, win_length, window, normalized, mode, floor, channels, width,
                                rolloff, out)

    def decode_clips_stft_long(self, clips, n_frames, sample_rate=44100, n_fft=2048, hop=512, win_length=None, window=None, normalized=False,
                               mode="complex", floor=1e-10, channels=1, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_stft_long: decode_clips_stft in everything -- arguments, definition, modes, out, valid,
        exceptions -- at n_fft 2048 or 4096 (hop 1 .. n_fft; win_length 1764 or 1920 is a shorter window inside 2048), computed
        as a two-stage transform by k_clip_stft_long."""
        return self._clips_stft("stft_long", clips, n_frames, sample_rate, n_fft, hop, win_length, window, normalized, mode, floor, channels,
                                width, rolloff, out)

    def decode_clips_cqt(self, clips, n_frames, sample_rate=22050, hop=512, fmin=CQT_FMIN, n_bins=84, bins_per_octave=12, filter_scale=1.0,
                         norm=1, scale=1, mode="magnitude", floor=1e-10, channels=1, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_cqt: clips = sequence of (mp3, StreamIndex, first sample at sample_rate) -> (out, valid):
        the constant-Q transform [K, C, n_bins, n_frames], frame f of a clip centred on sample start + f hop of the stream
        resampled as decode_clips_audio does (width, rolloff), zeros outside the stream and no reflection.  Bin k is at
        fmin 2^(k / bins_per_octave); its filter is the periodic Hann window of the odd length about
        filter_scale sample_rate / (f_k (2^(1 / bins_per_octave) - 1)), normalised by norm (0 none, 1 its sum, 2 its Euclidean
        norm) and scaled by scale (0 none, 1 sqrt(length), 2 length): norm=1, scale=1 is the convention of librosa's
        cqt(norm=1, scale=True), computed in full at the one rate -- not librosa's multirate approximation.  mode, floor, valid,
        out, RingReplay / MixedFormat as decode_clips_stft.  Synchronous."""
        spec = lambda f: (_cqt_spec(f, sample_rate, hop, fmin, n_bins, bins_per_octave, filter_scale, norm, scale, mode, floor, channels, width, rolloff), None)
        return self._clips_stft("cqt", clips, n_frames, sample_rate, None, hop, None, None, None, mode, floor, channels, width, rolloff, out,
                                nb=int(n_bins), spec_of=spec)

    def decode_clips_chroma(self, clips, n_frames, sample_rate=22050, hop=512, fmin=CQT_FMIN, n_bins=84, bins_per_octave=12, n_chroma=12,
                            base_class=0, filter_scale=1.0, norm=1, scale=1, quantity="magnitude", chroma_norm="max", norm_floor=1e-10, channels=0,
                            width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_chroma: clips as decode_clips_cqt takes them -> (out, valid): pitch-class profiles
        [K, C, n_chroma, n_frames] float32.  The constant-Q transform is decode_clips_cqt's at the same arguments, its
        magnitudes (quantity="magnitude") or powers ("power") bit for bit; bin k goes to class
        ((k + r // 2) // r + base_class) % n_chroma with r = bins_per_octave // n_chroma (base_class: the class of fmin, 0 where
        fmin is a C), the bins of a class are added in ascending order, and every frame is divided by
        max(its norm, norm_floor): chroma_norm "max" (librosa's norm=inf), "l1", "l2" or None.  A silent frame is exactly 0.
        The definition is this formula at the one rate, not librosa's multirate chroma_cqt.  valid, out, RingReplay /
        MixedFormat as decode_clips_stft.  Synchronous."""
        spec = lambda f: (_chroma_spec(f, sample_rate, hop, fmin, n_bins, bins_per_octave, n_chroma, base_class, filter_scale, norm, scale, quantity,
                                      chroma_norm, norm_floor, channels, width, rolloff), None)
        if (STFT_MODES.get(quantity) if isinstance(quantity, str) else quantity) not in (1, 2):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_chroma: quantity is \"magnitude\" or \"power\"")
        return self._clips_stft("chroma", clips, n_frames, sample_rate, None, hop, None, None, None, quantity, 0.0, channels, width, rolloff, out,
                                nb=int(n_chroma), spec_of=spec)

    def decode_clips_loudness(self, clips, n_samples, sample_rate=0, channels=0, target=None, peak_limit=0.0, dual_mono=False, width=0,
                              rolloff=0.0, out=None, momentary=None):
        """pdmp3_amd_bulk_decode_clips_loudness: clips, n_samples, sample_rate, channels, width, rolloff and out as
        decode_clips_audio takes them -> (audio, stats, valid).  stats float32 [K, 8] = integrated loudness L (LUFS, ITU-R
        BS.1770 / EBU R128), maximum momentary loudness M, sample peak P, the gain g, the relative threshold, the 400 ms blocks
        J, those above the absolute gate, those above both gates -- a torch tensor on the decoder's device, or a numpy array
        where out is one.  audio = decode_clips_audio's rows times g: g = 1 without a target (bit for bit that call's rows), else
        10^((target - L) / 20) with target in [-70, 0] LUFS, held to peak_limit / P where peak_limit > 0.  dual_mono: a mono
        clip counts twice (+3.01 dB).  momentary: None, or a float32 [K, Jmax] destination (torch on the device, or numpy) for
        the block loudnesses l_j, Jmax = max(0, n_samples // q - 3), q = (rate + 5) // 10.  A clip's filter starts from rest
        at its first sample.  Rows of stats belonging to clips that raise RingReplay / MixedFormat (.out, .stats, .valid) stay
        NaN.  With n_samples = 0 nothing is measured: stats stays NaN."""
        t, k = int(n_samples), len(clips)
        stats = _stats_like(out, (k, 8))
        mp = None
        if momentary is not None:
            mp = _aux_destination("momentary", momentary, k, lambda: _plan_field("loudness", loudness_plan, 6, clips, sample_rate, t), "Jmax")
        spec = lambda: (_loudness_spec(t, sample_rate, channels, target, peak_limit, dual_mono, width, rolloff), None)
        try:
            audio, valid = self._clips_call("loudness", clips, (t,), spec, channels, out, refused=(ValueError, OverflowError, TypeError),
                                            extra=(_address(stats), mp))
        except (RingReplay, MixedFormat) as e:
            e.stats = stats
            raise
        return audio, stats, valid

    def decode_clips_r128(self, clips, n_samples, sample_rate=0, channels=0, target=-23.0, peak_limit=10 ** (-1 / 20), limit_true_peak=True,
                          dual_mono=False, width=0, rolloff=0.0, out=None, momentary=None, short_term=None):
        """pdmp3_amd_bulk_decode_clips_r128: decode_clips_loudness with EBU R128's other descriptors and the gain held to the true
        peak -> (audio, stats, valid).  stats float32 [K, 16]: fields 0-7 as decode_clips_loudness's [L, M, P, g, Gamma, J, |A|,
        |Gt|], fields 8-15 = true peak TP (4x oversampled, libebur128's 49-tap interpolator), maximum short-term loudness Smax,
        loudness range LRA (LU), the range's relative threshold, the 3 s windows Js, those a second apart Jr, those above the
        range's absolute gate, those above both.  g = 10^((target - L) / 20), held to peak_limit / TP where peak_limit > 0 (to
        peak_limit / P with limit_true_peak=False, which makes fields 0-7, momentary and audio decode_clips_loudness's bit for
        bit); target=None: no gain.  The defaults are R128's: -23 LUFS under -1 dBTP.  momentary as there; short_term: None, or a
        float32 [K, Jsmax] destination for the window loudnesses S_j, Jsmax = max(0, n_samples // q - 29).  A clip's filters
        start from rest at its first sample.  Rows of stats belonging to clips that raise RingReplay / MixedFormat stay NaN."""
        t, k = int(n_samples), len(clips)
        stats = _stats_like(out, (k, 16))
        ptrs = [None if dst is None else _aux_destination(name, dst, k, lambda: _plan_field("r128", r128_plan, field, clips, sample_rate, t))
                for name, dst, field in (("momentary", momentary, 6), ("short_term", short_term, 9))]
        spec = lambda: (_r128_spec(t, sample_rate, channels, target, peak_limit, limit_true_peak, dual_mono, width, rolloff), None)
        try:
            audio, valid = self._clips_call("r128", clips, (t,), spec, channels, out, refused=(ValueError, OverflowError, TypeError),
                                            extra=(_address(stats), ptrs[0], ptrs[1]))
        except (RingReplay, MixedFormat) as e:
            e.stats = stats
            raise
        return audio, stats, valid

    def decode_clips_pitch(self, clips, n_frames, sample_rate=22050, frame_length=2048, hop=512, fmin=PITCH_FMIN, fmax=PITCH_FMAX, threshold=0.1,
                           out_mode="pitch", win_length=None, channels=1, width=0, rolloff=0.0, out=None):
        """pdmp3_amd_bulk_decode_clips_pitch: clips = sequence of (mp3, StreamIndex, first sample at sample_rate) -> (out, valid):
        YIN with librosa.yin's parameters on frames centred on sample start + f hop of the stream resampled as decode_clips_audio
        does (width, rolloff), zeros outside the stream and no reflection.  out_mode "pitch": float32 [K, C, 3, n_frames] -- f0 in
        Hz, the aperiodicity d'(tau*), the lag tau*; a frame of zeros is (0, 1, 0).  out_mode "curve": [K, C, tmax + 1, n_frames],
        the cumulative-mean-normalised difference d'(tau), tau = 0 .. tmax (pitch_lags gives tmax).  win_length None:
        frame_length // 2; hop None: frame_length // 4.  valid, out, RingReplay / MixedFormat as decode_clips_stft.  Synchronous."""
        f = int(n_frames)
        m = PITCH_MODES.get(out_mode) if isinstance(out_mode, str) else int(out_mode)
        spec = lambda: (_pitch_spec(f, sample_rate, frame_length, win_length, hop, fmin, fmax, threshold, m, channels, width, rolloff), None)
        if m not in (0, 1):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_pitch: out_mode is \"pitch\" or \"curve\"")
        rows = 3
        if m != 0:
            try:
                rows = pitch_lags(sample_rate, frame_length=frame_length, win_length=win_length, hop=hop, fmin=fmin, fmax=fmax)[1] + 1
            except (ValueError, OverflowError, TypeError):
                raise RuntimeError("pdmp3_amd_bulk_decode_clips_pitch: bad sample_rate, frame_length, win_length, hop, fmin or fmax")
        return self._clips_call("pitch", clips, (rows, f), spec, channels, out, refused=(ValueError, OverflowError, TypeError))

    def decode_clips_pyin(self, clips, n_frames, sample_rate=22050, channels=0, frame_length=2048, win_length=0, hop=0, fmin=PITCH_FMIN,
                          fmax=PITCH_FMAX, n_thresholds=100, beta=(2, 18), threshold_weights=None, boltzmann=2.0, resolution=0.1,
                          max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, fill=float("nan"), out_mode="pitch", out=None, width=0,
                          rolloff=0.0):
        """pdmp3_amd_bulk_decode_clips_pyin: clips as decode_clips_pitch takes them -> (out, valid): probabilistic YIN with
        librosa.pyin's parameters on the frames decode_clips_pitch reads (centred on sample start + f hop, zeros outside the stream,
        no reflection).  out_mode "pitch": float32 [K, C, 4, n_frames] -- f0 in Hz of the Viterbi path's pitch bin (`fill` on
        unvoiced frames; fill=None: the bin's frequency there too, librosa's fill_na=None), the voiced flag 1.0 / 0.0, the voiced
        probability, the bin.  out_mode "observation": [K, C, n_bins + 1, n_frames], the observation probabilities of the pitch
        bins with the voiced probability in the last row (pyin_plan gives n_bins).  beta: integers 1 .. 64, or pass
        threshold_weights (n_thresholds values).  The path depends on the clip's start: a clip's mode-"pitch" frames are not a
        slice of a longer clip's.  valid, out, RingReplay / MixedFormat as decode_clips_pitch.  Synchronous."""
        f = int(n_frames)
        m = PYIN_MODES.get(out_mode) if isinstance(out_mode, str) else out_mode
        if m not in (0, 1):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_pyin: out_mode is \"pitch\" or \"observation\"")
        kw = dict(sample_rate=sample_rate, channels=channels, frame_length=frame_length, win_length=win_length, hop=hop, fmin=fmin, fmax=fmax,
                  n_thresholds=n_thresholds, beta=beta, threshold_weights=threshold_weights, boltzmann=boltzmann, resolution=resolution,
                  max_transition_rate=max_transition_rate, switch_prob=switch_prob, no_trough_prob=no_trough_prob, fill=fill, out_mode=m,
                  width=width, rolloff=rolloff)
        rows = 4
        if m == 1:
            try:
                rows = pyin_plan(n_frames=f, **kw)["n_bins"] + 1
            except (ValueError, KeyError, OverflowError, TypeError):
                raise RuntimeError("pdmp3_amd_bulk_decode_clips_pyin: bad arguments")
        return self._clips_call("pyin", clips, (rows, f), lambda: _pyin_spec(f, **kw), channels, out, refused=(ValueError, KeyError, OverflowError, TypeError))

    def _clips_stft(self, call, clips, n_frames, sample_rate, n_fft, hop, win_length, window, normalized, mode, floor, channels, width, rolloff, out,
                    nb=None, spec_of=None):
        """the transform calls: `nb` bins (n_fft // 2 + 1) of n_frames frames, mode "complex" as complex64 or float32 [..., 2]; what
        the spec's making refuses is a RuntimeError like the library's own refusals"""
        f = int(n_frames)
        nb = int(n_fft) // 2 + 1 if nb is None else nb
        m = _enum(STFT_MODES, mode)
        if spec_of is not None:
            spec = lambda: spec_of(f)
        else:
            spec = lambda: _stft_spec(f, sample_rate, n_fft, hop, win_length, window, normalized, m, floor, channels, width, rolloff)
        return self._clips_call(call, clips, (nb, f, 2) if m == 0 else (nb, f), spec, channels, out, complex_ok=m == 0, refused=(ValueError, OverflowError))

    def decode_clips_tempogram(self, clips, n_frames, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, lag=1, max_size=1, win_length=384,
                               start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, out_mode="tempogram", out=None, f_min=0.0, f_max=0.0, scale="slaney",
                               norm="slaney", floor=1e-10, fft_win_length=None, fft_window=None, channels=1, width=0, rolloff=0.0):
        """pdmp3_amd_bulk_decode_clips_tempogram: clips as decode_clips_mel_long takes them -> (out, valid).  out_mode "onset":
        float32 [K, C, n_frames], librosa.onset.onset_strength(lag, max_size) of decode_clips_mel_long's log10 mel in dB, frame f
        centred on sample start + f hop, the frames in front of the clip the stream's own (no shift, no zero padding, no top_db:
        set floor for a fixed range); "tempogram": [K, C, win_length, n_frames], librosa.feature.tempogram's autocorrelation of
        the Hann-windowed envelope around every frame, normalised by lag 0; "tempo": [K, C, 4] -- librosa.feature.tempo's bpm
        (start_bpm, std_bpm, max_tempo), its lag in frames, the lag's score and the score's margin over every other lag.
        fft_win_length / fft_window are decode_clips_mel_long's win_length / window.  valid, out, the exceptions: as
        decode_clips_mel_long."""
        f, wt = int(n_frames), int(win_length)
        spec = lambda: _tempogram_spec(f, sample_rate, n_fft, hop, n_mels, lag, max_size, wt, start_bpm, std_bpm, max_tempo, out_mode, f_min, f_max,
                                       scale, norm, floor, fft_win_length, fft_window, channels, width, rolloff)
        if out_mode not in TEMPOGRAM_MODES:
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_tempogram: out_mode is \"onset\", \"tempogram\" or \"tempo\"")
        inner = {"onset": (f,), "tempogram": (wt, f), "tempo": (4,)}[out_mode]
        if out_mode == "tempogram" and out is None and not tempogram_check(sample_rate, win_length=wt):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_tempogram: bad win_length")
        return self._clips_call("tempogram", clips, inner, spec, channels, out, refused=(ValueError, KeyError, OverflowError, TypeError))

    def decode_clips_beats(self, clips, n_frames, sample_rate=22050, n_fft=2048, hop=512, n_mels=128, lag=1, max_size=1, win_length=384,
                           start_bpm=120.0, std_bpm=1.0, max_tempo=320.0, bpm=0.0, tightness=100.0, trim=True, out_mode="beats", out=None,
                           stats=None, f_min=0.0, f_max=0.0, scale="slaney", norm="slaney", floor=1e-10, fft_win_length=None, fft_window=None,
                           channels=1, width=0, rolloff=0.0):
        """pdmp3_amd_bulk_decode_clips_beats: clips and the envelope's arguments as decode_clips_tempogram takes them -> (out,
        stats, valid): librosa.beat.beat_track's dynamic programme (Ellis 2007) on decode_clips_tempogram's onset envelope, per
        clip and channel, over the clip's valid frames.  bpm 0: the tempo is decode_clips_tempogram(out_mode="tempo")'s and the
        period its lag; else the period is round(60 sample_rate / (hop bpm)).  out_mode "beats": float32 [K, C, 2, n_frames], row
        0 the beat mask, row 1 the beats' frames ascending with -1 behind them; "dp": [K, C, 2, n_frames], the cumulative score
        and the back-links; "score": [K, C, n_frames], the local score.  stats float32 [K, C, 8] (BEAT_STATS): the bpm used, the
        period, beats kept, beats before the trim, the tail frame, the envelope's norm, the trim's threshold, the frames that
        entered; -1 where not reached; a torch tensor on the decoder's device or a numpy array, as out; rows of clips that raise
        RingReplay / MixedFormat (.out, .stats, .valid) stay NaN.  n_frames <= 32768."""
        f, k = int(n_frames), len(clips)
        m = BEAT_MODES.get(out_mode) if isinstance(out_mode, str) else out_mode
        if m not in (0, 1, 2):
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_beats: out_mode is \"score\", \"dp\" or \"beats\"")
        c = int(channels) or (out.shape[1] if out is not None else 0)
        if not c:
            cs = set(ix.channels for _, ix, _ in clips if not ix.replay and ix.one_format)
            c = cs.pop() if len(cs) == 1 else 1
        if stats is None:
            stats = _stats_like(out, (k, c, 8))
        ok = (stats.is_contiguous() and str(stats.dtype) == "torch.float32") if hasattr(stats, "data_ptr") else \
            (stats.flags["C_CONTIGUOUS"] and stats.dtype == np.float32)
        assert ok and tuple(stats.shape) == (k, c, 8), "stats: float32 [K, C, 8], contiguous"
        sp = _address(stats)
        spec = lambda: _beat_spec(f, sample_rate, bpm, tightness, trim, m, n_fft=n_fft, hop=hop, n_mels=n_mels, lag=lag, max_size=max_size,
                                  win_length=win_length, start_bpm=start_bpm, std_bpm=std_bpm, max_tempo=max_tempo, f_min=f_min, f_max=f_max,
                                  scale=scale, norm=norm, floor=floor, fft_win_length=fft_win_length, fft_window=fft_window, channels=channels,
                                  width=width, rolloff=rolloff)
        try:
            out, valid = self._clips_call("beats", clips, (f,) if m == 0 else (2, f), spec, channels, out,
                                          refused=(ValueError, KeyError, OverflowError, TypeError), extra=(sp if k else None,))
        except (RingReplay, MixedFormat) as e:
            e.stats = stats
            raise
        return out, stats, valid

    def _clips_call(self, call, clips, inner, spec_of, channels, out, made=None, complex_ok=False, refused=(), extra=()):
        """What every decode_clips_<call> does around its spec: the channel count, `out` made when not given (float32
        [K, C] + `made`, which is `inner` unless given; complex_ok: complex64 without inner's last 2), the destination checked
        (_clip_destination), the clips' array, the library's call and its refusals as exceptions.  spec_of() -> (the call's spec,
        what has to stay alive beside it or None); an exception of the types `refused` from it becomes a RuntimeError.  extra: the
        library call's arguments between its spec and valid."""
        k = len(clips)
        c = int(channels)
        if not c:
            cs = set(ix.channels for _, ix, _ in clips if not ix.replay and ix.one_format)
            if len(cs) > 1:
                raise ValueError("decode_clips_%s: channels=0 and the clips' channel counts differ" % call)
            c = cs.pop() if cs else 1
        if out is None:
            import torch
            shape = (k, c) + tuple(inner[:-1] if complex_ok else inner if made is None else made)
            out = torch.zeros(shape, dtype=torch.complex64 if complex_ok else torch.float32, device=torch.device("cuda", torch.cuda.current_device()))
            torch.cuda.synchronize()
        base, s0, s1 = _clip_destination(out, k, c, inner, complex_ok)
        arr = (_AudioClip * max(k, 1))()
        keep = []                                      # (the arrays arr points into; never read: they live until the call is over)
        for i, (mp3, ix, start) in enumerate(clips):
            a = _as_u8(mp3)
            keep.append(a)
            arr[i] = _AudioClip(a.ctypes.data, len(mp3), ix.h, int(start), base + i * s0, max(int(s1), 0))
        try:
            spec, keep_spec = spec_of()                # (keep_spec: memory the spec points into; it lives until the call is over)
        except refused as e:
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_%s: %s" % (call, e))
        got = (C.c_longlong * max(k, 1))()
        rc = getattr(self.lib, "pdmp3_amd_bulk_decode_clips_" + call)(self.h, arr, k, C.byref(spec), *extra, got)
        valid = np.array(got[:k], dtype=np.int64)
        if rc in (PDMP3_BULK_REPLAY, PDMP3_BULK_MIXED_FORMAT):
            e = (RingReplay("the reference replays its input ring on a clip's stream (no finite output)") if rc == PDMP3_BULK_REPLAY else
                 MixedFormat("a clip's stream changes its sampling frequency or samples per frame (no time line in samples)"))
            e.valid, e.out = valid, out
            raise e
        if rc != 0:
            raise RuntimeError("pdmp3_amd_bulk_decode_clips_%s failed (a bad argument, a decoder without device Huffman, switches "
                               "that differ from an index's, or an engine failure)" % call)
        return out, valid

    def clip_stats(self):
        """-> (frames the decoder's clips kept, frames it decoded in front of them and threw away), over its life"""
        c, h = C.c_longlong(0), C.c_longlong(0)
        self.lib.pdmp3_amd_bulk_clip_stats(self.h, C.byref(c), C.byref(h))
        return c.value, h.value

    def parse_range(self, mp3, index, first, count, lookback=True):
        """parse-only decoders (host tests): pdmp3_amd_bulk_parse_range -> (first frame decoded, spectra, side) of the frames
        [that first frame, b): the records the host stage gives for the range by itself, halo included.  lookback=False: the
        synthesis halo alone."""
        a = _as_u8(mp3)
        f0 = C.c_longlong(0)
        args = (self.h, a.ctypes.data_as(C.c_void_p), len(mp3), index.h, int(first), int(count), 1 if lookback else 0)
        n = self.lib.pdmp3_amd_bulk_parse_range(*args, None, None, 0, C.byref(f0))     # (the first frame it would decode)
        if n == PDMP3_BULK_REPLAY:
            raise RingReplay("the reference replays its input ring on this stream (no finite output)")
        _, b = index.clamp(first, count)
        cap = max(b - f0.value, 0)
        sp = np.zeros((max(cap, 1), 2, 2, 576), dtype=np.int16)
        sd = np.zeros((max(cap, 1), 2, 2), dtype=SIDE_DTYPE)
        if cap:
            n = self.lib.pdmp3_amd_bulk_parse_range(*args, sp.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p), cap,
                                                    C.byref(f0))
            if n != cap:
                raise RuntimeError("pdmp3_amd_bulk_parse_range failed (%d)" % n)
        return f0.value, sp[:cap], sd[:cap]

    def parse(self, mp3):
        _, frames = scan_buffer(mp3, getattr(self, "iso", 0))
        cap = frames + 1                           # frames of a failed last read are parsed too
        sp = np.zeros((cap, 2, 2, 576), dtype=np.int16)
        sd = np.zeros((cap, 2, 2), dtype=SIDE_DTYPE)
        a = _as_u8(mp3)
        pcm_bytes = C.c_longlong(0)
        n = self.lib.pdmp3_amd_bulk_parse(self.h, a.ctypes.data_as(C.c_void_p), len(mp3), sp.ctypes.data_as(C.c_void_p),
                                          sd.ctypes.data_as(C.c_void_p), cap, C.byref(pcm_bytes))
        if n < 0:
            raise RuntimeError("pdmp3_amd_bulk_parse failed")
        return sp[:n], sd[:n], pcm_bytes.value


def parse_bits(mp3, iso=0, lsf=False):
    """Stage A of the bulk pipeline alone: per frame the side info (pdmp3_frame_bits) and the reservoir snapshot
    that pdmp3_hip_stream_submit_bits is given.  No GPU.  lsf=True: the scan a device-Huffman decoder runs, which with
    iso & ISO_LSF takes MPEG-2 LSF / 2.5 frames (the LSF form of pdmp3_frame_bits); False: the scan ends at the first one."""
    lib = load_library()
    lib.pdmp3_amd_bulk_set_quirks.argtypes = [C.c_void_p, C.c_uint]
    _, frames = scan_buffer(mp3, iso if lsf else 0)
    cap = frames + 1
    bits = np.zeros(cap, dtype=FRAME_BITS_DTYPE)
    res = np.zeros((cap, RESERVOIR_BYTES), dtype=np.uint8)
    assert FRAME_BITS_DTYPE.itemsize == 80
    a = _as_u8(mp3)
    h = lib.pdmp3_amd_bulk_new_parse_bits_lsf() if lsf else lib.pdmp3_amd_bulk_new_parse_bits()
    lib.pdmp3_amd_bulk_set_quirks(h, iso)
    pcm_bytes = C.c_longlong(0)
    n = lib.pdmp3_amd_bulk_parse_bits(h, a.ctypes.data_as(C.c_void_p), len(mp3), bits.ctypes.data_as(C.c_void_p),
                                      res.ctypes.data_as(C.c_void_p), cap, C.byref(pcm_bytes))
    lib.pdmp3_amd_bulk_delete(h)
    if n < 0:
        raise RuntimeError("pdmp3_amd_bulk_parse_bits failed")
    return bits[:n], res[:n], pcm_bytes.value


ROW_DESC_DTYPE = np.dtype([("row_off", "<u4"), ("s_off", "<u4"), ("top", "<u2"), ("back", "<u2"), ("up", "<u2"), ("reserved", "<u2")])


def parse_pool(mp3, iso=0, lsf=False):
    """Stage A alone in the compact form the engine is given: (bits, row descriptors, pool).  No GPU.  iso / lsf as for
    parse_bits."""
    lib = load_library()
    lib.pdmp3_amd_bulk_set_quirks.argtypes = [C.c_void_p, C.c_uint]
    _, frames = scan_buffer(mp3, iso if lsf else 0)
    cap = frames + 1
    bits = np.zeros(cap, dtype=FRAME_BITS_DTYPE)
    desc = np.zeros(cap, dtype=ROW_DESC_DTYPE)
    pool = np.zeros(cap * 2064 + 16384, dtype=np.uint8)
    a = _as_u8(mp3)
    h = lib.pdmp3_amd_bulk_new_parse_bits_lsf() if lsf else lib.pdmp3_amd_bulk_new_parse_bits()
    lib.pdmp3_amd_bulk_set_quirks(h, iso)
    used = C.c_size_t(0)
    lib.pdmp3_amd_bulk_parse_pool.restype = C.c_longlong
    lib.pdmp3_amd_bulk_parse_pool.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_size_t, C.POINTER(C.c_size_t)]
    n = lib.pdmp3_amd_bulk_parse_pool(h, a.ctypes.data_as(C.c_void_p), len(mp3), bits.ctypes.data_as(C.c_void_p),
                                      desc.ctypes.data_as(C.c_void_p), pool.ctypes.data_as(C.c_void_p), pool.nbytes, cap, C.byref(used))
    lib.pdmp3_amd_bulk_delete(h)
    if n < 0:
        raise RuntimeError("pdmp3_amd_bulk_parse_pool failed")
    return bits[:n], desc[:n], pool[:used.value]


class PinnedPCM:
    """int16 numpy view of a pinned host buffer (pdmp3_amd_pcm_alloc): decode into it and the GPU writes it directly"""

    def __init__(self, n_samples):
        self.lib = load_library()
        self.nbytes = max(2, int(n_samples) * 2)
        self.ptr = self.lib.pdmp3_amd_pcm_alloc(self.nbytes)
        if not self.ptr:
            raise MemoryError("pdmp3_amd_pcm_alloc(%d)" % self.nbytes)
        self.array = np.ctypeslib.as_array((C.c_int16 * (self.nbytes // 2)).from_address(self.ptr))

    def free(self):
        if self.ptr:
            self.array = None
            self.lib.pdmp3_amd_pcm_free(self.ptr)
            self.ptr = None


def corpus_assign(sizes, world):
    """pdmp3_amd_corpus_assign (include/pdmp3_bulk.h): device slot per file, largest first -- == sharding.assign_files; no GPU needed"""
    lib = load_library()
    n = len(sizes)
    arr = (C.c_size_t * n)(*[int(x) for x in sizes])
    out = (C.c_int * n)()
    lib.pdmp3_amd_corpus_assign.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.pdmp3_amd_corpus_assign.restype = None
    lib.pdmp3_amd_corpus_assign(arr, n, world, out)
    return list(out)


def corpus_decode(devices, mp3s, iso=0, threads=2, window_frames=0, host_huffman=False):
    """pdmp3_amd_corpus_decode: whole files over the devices of a node from C (one decoder and host thread per entry of
    `devices`) -> list of int16 arrays"""
    lib = load_library()
    n = len(mp3s)
    bufs = [_as_u8(m) for m in mp3s]
    totals = [max(0, scan_buffer(m, iso)[0]) for m in mp3s]
    outs = [np.empty(max(t, 2) // 2, dtype=np.int16) for t in totals]
    PP = C.c_void_p * n
    srcs = PP(*[b.ctypes.data for b in bufs])
    dsts = PP(*[o.ctypes.data for o in outs])
    sizes = (C.c_size_t * n)(*[len(m) for m in mp3s])
    caps = (C.c_size_t * n)(*[o.nbytes for o in outs])
    got = (C.c_longlong * n)()
    dev = (C.c_int * len(devices))(*[int(d) for d in devices])
    lib.pdmp3_amd_corpus_decode.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint, C.c_int, C.c_int, C.c_int]
    rc = lib.pdmp3_amd_corpus_decode(dev, len(devices), srcs, sizes, n, dsts, caps, got, iso, threads, window_frames, int(host_huffman))
    if rc != 0:
        raise RuntimeError("pdmp3_amd_corpus_decode failed")
    assert list(got) == totals, (list(got), totals)
    return [o[:t // 2] for o, t in zip(outs, totals)]
