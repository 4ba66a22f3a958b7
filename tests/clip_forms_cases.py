"""The arguments and cases of the mel, fbank, mfcc and stft comparisons with the definition on the GPU (tests/test_gpu_clip_mel.py,
_fbank.py, _mfcc.py, _stft.py): what the suite ran on the device before the EDGES tables of tests/clip_*_ref.py.  They stand here,
beside tests/clip_forms_draws.py, because tests/test_clip_forms_host.py reads them without a GPU."""
import numpy as np

SIX = ["mixed/mono-stereo", "48k", "32k", "22k", "16k-mono", "8k"]     # one stream of every rate

# ---- decode_clips_mel ----
MEL_P16 = dict(sample_rate=16000, n_fft=400, hop=160, n_mels=80, scale="slaney", norm="slaney", channels=1)
MEL_P24 = dict(sample_rate=24000, n_fft=512, hop=128, n_mels=128, scale="htk", norm=None, channels=2)
MEL_P48 = dict(sample_rate=0, n_fft=1024, hop=1024, n_mels=40, scale="slaney", norm="slaney", channels=2)      # the own rate (the 48 kHz stream)
MEL_CASES = {
    "16k-mono-batch": (MEL_P16, SIX, 70),
    "24k-stereo-htk": (MEL_P24, ["48k", "22k", "mixed/mono-stereo"], 45),
    "own-rate-1024": (MEL_P48, ["48k"], 21),
}

# ---- decode_clips_fbank ----
FBANK_P16 = dict(sample_rate=16000, win_length=400, hop=160, num_mel_bins=80, channels=1)
FBANK_P8 = dict(sample_rate=8000, win_length=200, hop=80, num_mel_bins=23, channels=1, use_energy=True, htk_compat=True, scale=32768.0)
FBANK_POWN = dict(sample_rate=0, win_length=1024, hop=480, num_mel_bins=80, channels=2)          # the own rate (the 48 kHz stream), stereo
FBANK_PEQ = dict(sample_rate=16000, win_length=400, hop=160, num_mel_bins=40, channels=1, round_to_power_of_two=False)
FBANK_CASES = {
    "16k-mono-batch": (FBANK_P16, SIX, 70),
    "8k-energy-htk-int16": (FBANK_P8, ["48k", "22k", "8k"], 45),
    "own-rate-1024-stereo": (FBANK_POWN, ["48k"], 21),
    "n-equals-nw": (FBANK_PEQ, ["32k", "16k-mono"], 40),
}
FBANK_VARIANTS = {
    "hanning": dict(window_type="hanning"),
    "hamming": dict(window_type="hamming"),
    "rectangular": dict(window_type="rectangular"),
    "blackman": dict(window_type="blackman"),
    "blackman-0.4": dict(window_type="blackman", blackman_coeff=0.4),
    "rho-0": dict(preemphasis_coefficient=0.0),
    "rho-1": dict(preemphasis_coefficient=1.0),
    "no-dc-removal": dict(remove_dc_offset=False, use_energy=True),
    "energy-first-floor": dict(use_energy=True, energy_floor=0.5),
    "energy-power": dict(use_energy=True, use_log_fbank=False),
    "subtract-mean": dict(subtract_mean=True),
    "subtract-mean-energy-power": dict(subtract_mean=True, use_energy=True, use_log_fbank=False, htk_compat=True),
    "band": dict(low_freq=300.0, high_freq=-400.0, num_mel_bins=23),
}

# ---- decode_clips_mfcc ----
MFCC_P16 = dict(sample_rate=16000, win_length=400, hop=160, num_mel_bins=23, num_ceps=13, channels=1)
MFCC_P8 = dict(sample_rate=8000, win_length=200, hop=80, num_mel_bins=23, num_ceps=13, channels=1, use_energy=True, scale=32768.0)
MFCC_POWN = dict(sample_rate=0, win_length=1024, hop=480, num_mel_bins=80, num_ceps=40, channels=2)         # the own rate (the 48 kHz stream), stereo
MFCC_SMALL_N = dict(sample_rate=8000, win_length=16, hop=16, num_mel_bins=40, num_ceps=40, channels=1, low_freq=0.0)  # cepstra [tile][49], powers [tile][18]
MFCC_CASES = {
    # parameters, streams, frames, destinations
    "16k-23-bands-13-cepstra": (MFCC_P16, SIX, 70, ("device", "numpy")),                       # three tiles of 32, the last partial
    "80-bands-80-cepstra": (dict(MFCC_P16, num_mel_bins=80, num_ceps=80), ["48k", "22k"], 40, ("device",)),   # five column tiles over four waves
    "17-cepstra": (dict(MFCC_P16, num_ceps=17), ["32k", "8k"], 40, ("device",)),               # a partial column tile
    "1-cepstrum": (dict(MFCC_P16, num_ceps=1), ["32k", "8k"], 40, ("device",)),
    "8k-energy-first-int16": (MFCC_P8, ["48k", "8k"], 45, ("device",)),
    "8k-energy-last-htk-int16": (dict(MFCC_P8, htk_compat=True), ["48k", "8k"], 45, ("device",)),
    "htk-sqrt-2": (dict(MFCC_P16, htk_compat=True), ["48k", "16k-mono"], 40, ("device",)),
    "no-lifter": (dict(MFCC_P16, cepstral_lifter=0.0), ["48k", "16k-mono"], 40, ("device",)),
    "own-rate-1024-stereo": (MFCC_POWN, ["48k"], 21, ("device",)),
    "n-equals-nw": (dict(MFCC_P16, num_mel_bins=40, num_ceps=20, round_to_power_of_two=False), ["32k", "16k-mono"], 40, ("device",)),
    "cepstra-outgrow-powers": (MFCC_SMALL_N, ["48k", "8k"], 70, ("device",)),
}

# ---- decode_clips_stft ----
W301 = (np.random.default_rng(301).random(301, dtype=np.float32) * np.float32(1.5) - np.float32(0.25)).astype(np.float32)
STFT_P16 = dict(sample_rate=16000, n_fft=400, hop=160, channels=1)
STFT_P24 = dict(sample_rate=24000, n_fft=512, hop=128, channels=2, win_length=301, window=W301, normalized=True)
STFT_P48 = dict(sample_rate=0, n_fft=1024, hop=1024, channels=2)               # the own rate (the 48 kHz stream); the static array
STFT_P48H = dict(sample_rate=0, n_fft=1024, hop=512, channels=1)               # a tile of 16 frames inside 64 KB
STFT_P8 = dict(sample_rate=16000, n_fft=16, hop=1, channels=1)
STFT_CASES = {
    "16k-mono-batch": (STFT_P16, SIX, 70),
    "24k-stereo-own-window": (STFT_P24, ["48k", "22k", "mixed/mono-stereo"], 45),
    "own-rate-1024": (STFT_P48, ["48k"], 21),
    "own-rate-1024-hop-512": (STFT_P48H, ["48k"], 21),
    "n16-hop1": (STFT_P8, ["32k"], 40),
}
