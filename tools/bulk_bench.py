#!/usr/bin/env python3
"""Throughput of the bulk pipeline (include/pdmp3_bulk.h) on a long synthetic
stream (44.1 kHz joint stereo 320 kbps).  Host stages alone
(--parse-only, runs anywhere) or end to end on the GPU box.

  python tools/bulk_bench.py --frames 137813 --threads 1,8,32,64

--lsf VERSION (1 = MPEG-2 LSF, 2 = MPEG-2.5) with --sfreq: an LSF stream instead (joint stereo, 64 kbps; PDMP3_ISO_LSF on
every decoder), e.g. an hour at 22.05 kHz:

  python tools/bulk_bench.py --lsf 1 --sfreq 0 --frames 137812 --threads 4 --device-out [--host-huffman]

--clips K --clip-frames F: K clips of F frames at random places (fixed seed) in the C4 corpus -- or, with --c3, in the C3 hour --
into device memory with pdmp3_amd_bulk_decode_clips, against decoding the files whole and slicing (see clips()):

  python tools/bulk_bench.py --clips 64 --clip-frames 191
  python tools/bulk_bench.py --clips 1 --clip-frames 191 --c3
  python tools/bulk_bench.py --clips 64 --clip-frames 191 --audio 16000 [--mono]     (clips_audio(): the float batch at one rate)
  python tools/bulk_bench.py --clips 64 --clip-frames 1149 --mel                     (clips_mel(): log-mel features, 30 s a clip)
  python tools/bulk_bench.py --clips 64 --clip-frames 1149 --stft                    (clips_stft(): the short-time Fourier transform)
  python tools/bulk_bench.py --stft-long                                             (clips_stft(long=True): 64 clips of 30 s at 44.1 kHz, n_fft 2048, hop 512)
  python tools/bulk_bench.py --clips 64 --clip-frames 1149 --fbank                   (clips_fbank(): Kaldi-style filterbank features)
  python tools/bulk_bench.py --clips 64 --clip-frames 1149 --mfcc                    (clips_mfcc(): Kaldi-style MFCC features)
"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from math import gcd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")     # before HIP starts (torch brings it up): see host/stream_api.c shared_ctx_on


def clip_corpus(args, api):
    """what the clip modes cut their clips from: the C3 file (python -m pdmp3_amd.packer c3) with --c3, else the C4 corpus
    (python -m pdmp3_amd.packer c4) -> (files, a StreamIndex of each, close() for the indices)"""
    from pdmp3_amd.packer import packer
    from pdmp3_amd.packer.__main__ import c4_specs
    specs = [dict(n_frames=137813, seed=0xC3, sfreq=0, mode=1, mode_ext=2, bitrate_index=14)] if args.c3 else c4_specs(4096)
    files = [np.frombuffer(packer.generate(**s), dtype=np.uint8) for s in specs]
    ixs = [api.StreamIndex(f) for f in files]

    def close():
        for ix in ixs:
            ix.close()
    return files, ixs, close


def corpus_name(args, files):
    return "C3 file" if args.c3 else "C4 corpus (%d files, >= 4096 frames each)" % len(files)


def clip_selection(args, ixs, first=0, margin=0):
    """--clips picks of (file, frame) from --seed: the file, then a frame from `first` on that leaves --clip-frames + margin
    frames behind it where the file has them"""
    rng = random.Random(args.seed)
    sel = []
    for _ in range(args.clips):
        i = rng.randrange(len(ixs))
        sel.append((i, rng.randrange(first, max(first + 1, ixs[i].frames - args.clip_frames - margin))))
    return sel


def clip_start(ix, frame, rate, floor_at=0):
    """the first sample at `rate` at or behind the first sample of frame `frame` of the stream, floor_at at the least"""
    g = gcd(ix.rate, rate) if ix.rate else 1
    m, l = (ix.rate // g, rate // g) if ix.rate else (1, 1)
    return max(-((-frame * ix.frame_samples * l) // m), floor_at)


def time_routes(routes, warmup_runs, runs, after_first=None):
    """routes [(name, callable)] run in turn warmup_runs + runs times, every round starting one route later
    -> {name: [seconds of each round behind the warm-up]}; after_first() once, behind the first round"""
    n = len(routes)
    times = {name: [] for name, _ in routes}
    for r in range(warmup_runs + runs):
        for name, fn in routes[r % n:] + routes[:r % n]:
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= warmup_runs:
                times[name].append(dt)
        if r == 0 and after_first is not None:
            after_first()
    return times


def route_stats(times, K):
    """time_routes's result -> the result line's entry of every route"""
    return {name: {"seconds": {"median": round(statistics.median(ts), 6), "min": round(min(ts), 6), "max": round(max(ts), 6)},
                   "clips_per_s": {"median": round(K / statistics.median(ts), 1)}} for name, ts in times.items()}


def c4(args, api):
    """files dealt largest-first to JOBS decoders (pdmp3_amd.sharding.assign_files), each on its own host thread
    with its own HIP streams; decoders and output buffers exist before the clock starts"""
    import threading
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_gpu_corpus import _c4_files
    from pdmp3_amd.sharding import assign_files
    files = _c4_files(4096, 64, 12)
    files = [np.frombuffer(f, dtype=np.uint8) for f in files + files[:10]]
    sizes = [api.scan_buffer(f) for f in files]
    pins = [api.PinnedPCM(max(b, 2) // 2) for b, _ in sizes] if args.pinned else []
    outs = [p.array for p in pins] if args.pinned else [np.zeros(max(b, 2) // 2, dtype=np.int16) for b, _ in sizes]
    plan = assign_files([len(f) for f in files], args.c4)
    import torch
    ngpu = max(1, min(args.gpus, torch.cuda.device_count()))
    decs = [api.BulkDecoder(threads=2, window_frames=args.window, host_huffman=args.host_huffman, device=j % ngpu)
            for j in range(args.c4)]

    douts = [torch.empty(max(b, 2) // 2, dtype=torch.int16, device="cuda:%d" % (0)) for b, _ in sizes] if args.device_out else None

    calls = {}

    def work(j):
        t_calls = []
        for i in plan[j]:                                  # back to back, one wait at the end
            t0 = time.perf_counter()
            if douts is not None:
                got, _, _ = decs[j].decode_into_device(files[i], douts[i], wait=False)
            else:
                got, _, _ = decs[j].decode_into_async(files[i], outs[i])
            t_calls.append(time.perf_counter() - t0)
            assert got == sizes[i][0]
        t0 = time.perf_counter()
        decs[j].wait()
        calls[j] = (t_calls, time.perf_counter() - t0)
    best = None
    for _ in range(args.reps + 1):                      # first pass = warm-up
        ts = [threading.Thread(target=work, args=(j,)) for j in range(args.c4)]
        t0 = time.perf_counter()
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    for d in decs:
        d.close()
    if os.environ.get("BULK_BENCH_VERBOSE"):               # the last pass: where a decoder's time went
        for j, (tc, tw) in sorted(calls.items()):
            print("decoder %d: %d files, calls %.2f ms in all (median %.0f us, longest %.0f us), final wait %.2f ms" %
                  (j, len(tc), sum(tc) * 1e3, sorted(tc)[len(tc) // 2] * 1e6, max(tc) * 1e6, tw * 1e3), file=sys.stderr)
    frames = sum(fr for _, fr in sizes)
    print(json.dumps({"workload": "C4: %d files, %d frames, mono/stereo/joint x 32/44.1/48 kHz x CBR/VBR x block mixes" % (len(files), frames),
                      "decoders": args.c4, "gpus": ngpu, "seconds": round(best, 4), "frames_per_s": round(frames / best, 1),
                      "mp3_bytes": int(sum(len(f) for f in files)), "pcm_bytes": int(sum(b for b, _ in sizes)),
                      "mode": "host Huffman" if args.host_huffman else "device Huffman", "pcm": "device" if args.device_out else "pinned" if args.pinned else "pageable",
                      "host_cpus": os.cpu_count()}))


def clips(args, api):
    """K clips of F frames at random places (fixed seed) in the C4 corpus (python -m pdmp3_amd.packer c4) -- or, with --c3,
    in the C3 file (python -m pdmp3_amd.packer c3) -- into one [K, stride] int16 tensor in device memory, two ways, run
    after run in turn: pdmp3_amd_bulk_decode_clips (indices built beforehand, their build timed on its own), and what there
    was without it -- every file a clip falls in decoded whole with decode_into_device (asynchronously, back to back) and the
    clips sliced out of it on the device.  The two results are compared once, bit for bit.  Medians of --runs runs."""
    import random
    import statistics
    import torch
    from pdmp3_amd.packer import packer
    from pdmp3_amd.packer.__main__ import c4_specs
    t0 = time.perf_counter()
    if args.c3:
        specs = [dict(n_frames=137813, seed=0xC3, sfreq=0, mode=1, mode_ext=2, bitrate_index=14)]
    else:
        specs = c4_specs(4096)
    files = [np.frombuffer(packer.generate(**s), dtype=np.uint8) for s in specs]
    t_gen = time.perf_counter() - t0
    t_ix, ixs = [], []
    for f in files:
        t0 = time.perf_counter()
        ixs.append(api.StreamIndex(f))
        t_ix.append(time.perf_counter() - t0)
    rng = random.Random(args.seed)
    K, F = args.clips, args.clip_frames
    sel = []
    for _ in range(K):
        i = rng.randrange(len(files))
        sel.append((i, rng.randrange(max(1, ixs[i].frames - F))))
    spans = [(int(ixs[i].pcm_offsets[a]) // 2, int(ixs[i].pcm_offsets[min(a + F, ixs[i].frames)]) // 2) for i, a in sel]
    stride = max(hi - lo for lo, hi in spans)
    dev = "cuda:0"
    out_c = torch.zeros((K, stride), dtype=torch.int16, device=dev)
    out_w = torch.zeros((K, stride), dtype=torch.int16, device=dev)
    need = sorted(set(i for i, _ in sel))
    whole = {i: torch.empty(max(int(ixs[i].pcm_offsets[-1]), 2) // 2, dtype=torch.int16, device=dev) for i in need}
    dec_c = api.BulkDecoder(threads=args.clip_threads)
    dec_w = api.BulkDecoder(threads=args.clip_threads)
    batch = [(files[i], ixs[i], a, F) for i, a in sel]
    torch.cuda.synchronize()

    def clip_route():
        dec_c.decode_clips(batch, out_c)

    def whole_route():
        for i in need:
            dec_w.decode_into_device(files[i], whole[i], wait=False)
        dec_w.wait()
        for k, (i, _) in enumerate(sel):
            lo, hi = spans[k]
            out_w[k, :hi - lo].copy_(whole[i][lo:hi])
        torch.cuda.synchronize()

    times = {"clips": [], "whole files": []}
    halo = None
    for r in range(args.warmup_runs + args.runs):
        order = [("clips", clip_route), ("whole files", whole_route)]
        if r % 2:
            order.reverse()
        for name, fn in order:
            h0 = dec_c.clip_stats()[1]
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if name == "clips" and halo is None:
                halo = (dec_c.clip_stats()[1] - h0) / K
            if r >= args.warmup_runs:
                times[name].append(dt)
        if r == 0:
            assert torch.equal(out_c, out_w), "clips differ from the whole-file decodes sliced"
    dec_c.close()
    dec_w.close()
    kept = sum(min(a + F, ixs[i].frames) - a for i, a in sel)
    mb = [len(f) / 1e6 for f in files]
    res = {"workload": "%d clips of %d frames: %s" % (K, F, "C3 file (137813 frames, 320 kbps joint stereo)" if args.c3 else
                                                       "C4 corpus (%d files, >= 4096 frames each)" % len(files)),
           "destination": "device memory ([K, stride] int16 tensor)", "runs": args.runs, "kept_frames": kept,
           "files_decoded_whole": len(need), "whole_file_frames": int(sum(ixs[i].frames for i in need)),
           "halo_frames_per_clip": round(halo, 2), "packer_s": round(t_gen, 2),
           "index_build_ms_per_file": {"median": round(statistics.median(t_ix) * 1e3, 3), "min": round(min(t_ix) * 1e3, 3),
                                       "max": round(max(t_ix) * 1e3, 3)},
           "index_build_ms_per_mb": round(sum(t_ix) * 1e3 / sum(mb), 3), "host_cpus": os.cpu_count()}
    for name, ts in times.items():
        res[name] = {"seconds": {"median": round(statistics.median(ts), 6), "min": round(min(ts), 6), "max": round(max(ts), 6)},
                     "clips_per_s": {"median": round(K / statistics.median(ts), 1), "min": round(K / max(ts), 1), "max": round(K / min(ts), 1)},
                     "kept_frames_per_s": {"median": round(kept / statistics.median(ts), 1), "min": round(kept / max(ts), 1),
                                           "max": round(kept / min(ts), 1)}}
    w = times["whole files"]
    res["clip_route_wins_by_more_than_the_whole_route_spread"] = bool(statistics.median(w) - statistics.median(times["clips"]) > max(w) - min(w))
    for ix in ixs:
        ix.close()
    print(json.dumps(res))


def clips_audio(args, api):
    """--clips K --clip-frames F --audio RATE [--mono]: the clips of clips() (same seed, same places) as one float32 batch
    [K, C, T] at RATE in device memory, T = the length of F MPEG-1 frames at 44.1 kHz, three ways, run after run in turn:
    pdmp3_amd_bulk_decode_clips_audio; the plain clip call on the same clips (int16, every clip at its own rate: what there was
    before); and the plain clip call followed by the chain of torch kernels the audio call replaces (de-interleave, / 32768,
    mean, one strided conv1d per source rate with the same filter table, pad).  The chain starts every clip at its frame's first
    sample, the audio call at the first output sample at or behind it: the two are not compared value by value (the tests
    check the audio call against the definition).  Medians of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, C = args.clips, args.clip_frames, args.audio, 1 if args.mono else 2
    sel = clip_selection(args, ixs)
    T = F * 1152 * rate // 44100
    spans = [(int(ixs[i].pcm_offsets[a]) // 2, int(ixs[i].pcm_offsets[min(a + F, ixs[i].frames)]) // 2) for i, a in sel]
    stride = max(hi - lo for lo, hi in spans)
    dev = "cuda:0"
    out_p = torch.zeros((K, stride), dtype=torch.int16, device=dev)
    out_a = torch.zeros((K, C, T), dtype=torch.float32, device=dev)
    out_t = torch.zeros((K, C, T), dtype=torch.float32, device=dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    plain = [(files[i], ixs[i], a, F) for i, a in sel]
    audio = [(files[i], ixs[i], clip_start(ixs[i], a, rate)) for i, a in sel]
    kern = {}
    for r in sorted(set(ixs[i].rate for i, _ in sel)):
        if r and r != rate:
            tab, d0 = api.audio_table(r, rate)
            g = gcd(r, rate)
            m, l = r // g, rate // g
            w = np.zeros((l, 1, (l - 1) * m // l + tab.shape[1]), dtype=np.float32)
            for p in range(l):
                w[p, 0, p * m // l:p * m // l + tab.shape[1]] = tab[p * m % l]
            kern[r] = (torch.from_numpy(w).to(dev), m, l, -d0)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, C, out=out_a)

    def plain_route():
        dec.decode_clips(plain, out_p)

    def torch_route():
        dec.decode_clips(plain, out_p)
        out_t.zero_()
        for k, (i, a) in enumerate(sel):
            ix = ixs[i]
            if not ix.frames:
                continue
            lo, hi = spans[k]
            x = out_p[k, :hi - lo]
            x = (x.view(-1, 2).t() if ix.channels == 2 else x.view(1, -1)).to(torch.float32) / 32768.0   # (the corpus has no mono frames inside stereo files)
            if C == 1:
                x = x.mean(dim=0, keepdim=True)
            elif x.shape[0] == 1:
                x = x.expand(2, -1)
            if ix.rate != rate:
                w, m, l, left = kern[ix.rate]
                x = torch.nn.functional.pad(x.unsqueeze(1), (left, w.shape[2]))
                x = torch.nn.functional.conv1d(x, w, stride=m).transpose(1, 2).reshape(x.shape[0], -1)
            n = min(T, x.shape[1])
            out_t[k, :, :n] = x[:, :n]
        torch.cuda.synchronize()

    routes = [("audio clips", audio_route), ("plain clips", plain_route), ("plain clips + torch chain", torch_route)]
    times = {name: [] for name, _ in routes}
    frames = {}
    for r in range(args.warmup_runs + args.runs):
        for name, fn in routes[r % 3:] + routes[:r % 3]:
            c0 = dec.clip_stats()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            c1 = dec.clip_stats()
            frames[name] = {"kept": c1[0] - c0[0], "halo": c1[1] - c0[1]}
            if r >= args.warmup_runs:
                times[name].append(dt)
    dec.close()
    res = {"workload": "%d clips of %d frames' length (%d samples at %d Hz, %d channel(s)): %s" % (
               K, F, T, rate, C, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "host_cpus": os.cpu_count()}
    for name, entry in route_stats(times, K).items():
        res[name] = dict(entry, frames_decoded=frames[name])
    close()
    print(json.dumps(res))


def clips_mel(args, api):
    """--clips K --clip-frames F --mel: the clips of clips() (same seed, same places), F MPEG-1 frames' length each, as log-mel
    features [K, 1, 80, frames] at 16 kHz mono (n_fft 400, hop 160, Slaney, log10) in device memory, three ways, run after run in
    turn: (a) pdmp3_amd_bulk_decode_clips_audio for the samples the frames read (the call the feature call makes itself: what
    there was before); (b) (a) followed by the chain of torch kernels the feature call replaces -- torch.stft with the same
    window, abs() ** 2, a matmul with the same filterbank, log10; a dense matmul against the same DFT table where torch.stft
    cannot run --; (c) pdmp3_amd_bulk_decode_clips_mel.  (b) and (c) are compared once (largest difference of the log10 values,
    printed, not asserted: the tests check (c) against the definition).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, n_fft, hop, n_mels, floor = args.clips, args.clip_frames, 16000, 400, 160, 80, 1e-10
    sel = clip_selection(args, ixs)
    Fm = (F * 1152 * rate // 44100) // hop
    T = (Fm - 1) * hop + n_fft
    dev = "cuda:0"
    mel, audio = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, n_fft // 2)                        # (no leading zeros: (a)'s rows start at start - n_fft / 2)
        mel.append((files[i], ixs[i], start))
        audio.append((files[i], ixs[i], start - n_fft // 2))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_t = torch.zeros((K, 1, n_mels, Fm), dtype=torch.float32, device=dev)
    out_m = torch.zeros((K, 1, n_mels, Fm), dtype=torch.float32, device=dev)
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float32, device=dev)
    fb = torch.from_numpy(api.mel_filterbank(rate, n_fft, n_mels)).to(dev)
    kp = (n_fft // 2 + 1 + 15) // 16 * 16
    table = torch.from_numpy(api.mel_dft_table(n_fft)[:n_fft]).to(dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    how = {"stft": "torch.stft"}

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def torch_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)
        y = out_a[:, 0]
        if how["stft"] == "torch.stft":
            try:
                p = torch.stft(y, n_fft, hop_length=hop, window=window, center=False, return_complex=True).abs() ** 2      # [K, bins, Fm]
            except Exception as e:                      # noqa: BLE001  (no FFT library on this build)
                how["stft"] = "dense matmul against the DFT table (torch.stft: %s)" % type(e).__name__
        if how["stft"] != "torch.stft":
            x = y.unfold(1, n_fft, hop) @ table                                                                          # [K, Fm, 2 Kp]
            p = (x[:, :, :n_fft // 2 + 1] ** 2 + x[:, :, kp:kp + n_fft // 2 + 1] ** 2).transpose(1, 2)
        out_t[:, 0] = torch.log10(torch.clamp(fb @ p, min=floor))
        torch.cuda.synchronize()

    def mel_route():
        dec.decode_clips_mel(mel, Fm, rate, n_fft, hop, n_mels, floor=floor, out=out_m)

    routes = [("audio clips", audio_route), ("audio clips + torch chain", torch_route), ("mel clips", mel_route)]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(diff=float((out_t - out_m).abs().max())))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as %d frames x %d bands at %d Hz mono (n_fft %d, hop %d, log10): %s" % (
               K, F, Fm, n_mels, rate, n_fft, hop, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "torch_chain": how["stft"],
           "largest_difference_of_the_two_log10_results": seen["diff"], "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    b = times["audio clips + torch chain"]
    res["mel_minus_audio_ms"] = round((statistics.median(times["mel clips"]) - statistics.median(times["audio clips"])) * 1e3, 3)
    res["mel_not_above_torch_chain_by_more_than_its_spread"] = bool(statistics.median(times["mel clips"]) - statistics.median(b) <= max(b) - min(b))
    close()
    print(json.dumps(res))


def clips_stft(args, api, long=False):
    """--stft-long (long): the same three routes for 64 clips of 30 s (--clips / --clip-frames change that) at 44.1 kHz mono,
    n_fft 2048, hop 512, complex, with pdmp3_amd_bulk_decode_clips_stft_long as route (c).  Asserts nothing.
    --clips K --clip-frames F --stft: the clips of clips() (same seed, same places), F MPEG-1 frames' length each, as their
    short-time Fourier transform [K, 1, 201, frames] complex64 at 16 kHz mono (n_fft 400, hop 160, periodic Hann) in device
    memory, three ways, run after run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the samples the frames read (the call
    the new call makes itself); (b) (a) followed by torch.stft on the device (the same window, center=False on the padded
    span): what a loader does today; a dense matmul against the same table where torch.stft cannot run; (c)
    pdmp3_amd_bulk_decode_clips_stft.  (b) and (c) are compared once (largest difference, printed, not asserted: the tests
    check (c) against the definition).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, n_fft, hop = args.clips, args.clip_frames, 16000, 400, 160
    if long:
        rate, n_fft, hop = 44100, 2048, 512
    bins = n_fft // 2 + 1
    sel = clip_selection(args, ixs)
    Fm = (F * 1152 * rate // 44100) // hop
    T = (Fm - 1) * hop + n_fft
    dev = "cuda:0"
    stft, audio = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, n_fft // 2)                        # (no leading zeros: (a)'s rows start at start - n_fft / 2)
        stft.append((files[i], ixs[i], start))
        audio.append((files[i], ixs[i], start - n_fft // 2))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_t = torch.zeros((K, 1, bins, Fm), dtype=torch.complex64, device=dev)
    out_s = torch.zeros((K, 1, bins, Fm), dtype=torch.complex64, device=dev)
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float32, device=dev)
    kp = (bins + 15) // 16 * 16
    if long:                                            # (the direct table at this length, for the fallback of route (b) alone)
        ang = 2.0 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(kp)[None, :]) % n_fft) / n_fft
        w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))[:, None]
        table = torch.from_numpy(np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1).astype(np.float32)).to(dev)
    else:
        table = torch.from_numpy(api.stft_table(n_fft)[:n_fft]).to(dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    how = {"stft": "torch.stft"}

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def torch_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)
        y = out_a[:, 0]
        if how["stft"] == "torch.stft":
            try:
                out_t[:, 0] = torch.stft(y, n_fft, hop_length=hop, window=window, center=False, return_complex=True)       # [K, bins, Fm]
            except Exception as e:                      # noqa: BLE001  (no FFT library on this build)
                how["stft"] = "dense matmul against the table (torch.stft: %s)" % type(e).__name__
        if how["stft"] != "torch.stft":
            x = y.unfold(1, n_fft, hop) @ table                                                                          # [K, Fm, 2 Kp]
            out_t[:, 0] = torch.complex(x[:, :, :bins], x[:, :, kp:kp + bins]).transpose(1, 2)
        torch.cuda.synchronize()

    def stft_route():
        (dec.decode_clips_stft_long if long else dec.decode_clips_stft)(stft, Fm, rate, n_fft, hop, out=out_s)

    routes = [("audio clips", audio_route), ("audio clips + torch.stft", torch_route), ("stft clips", stft_route)]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(diff=float((out_t - out_s).abs().max())))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as %d frames x %d bins complex64 at %d Hz mono (n_fft %d, hop %d): %s" % (
               K, F, Fm, bins, rate, n_fft, hop, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "torch_route": how["stft"],
           "largest_difference_of_the_two_results": seen["diff"], "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    res["stft_minus_audio_ms"] = round((med["stft clips"] - med["audio clips"]) * 1e3, 3)
    res["torch_minus_audio_ms"] = round((med["audio clips + torch.stft"] - med["audio clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(spread * 1e3, 3)
    res["stft_cheaper_than_torch_stft_by_more_than_the_spread"] = bool(med["audio clips + torch.stft"] - med["stft clips"] > spread)
    close()
    print(json.dumps(res))


def clips_mel_long(args, api):
    """--mel-long: 64 clips of 30 s (--clips / --clip-frames change that) at 44.1 kHz mono as 128 log10-mel bands x 2583 frames
    (n_fft 2048, hop 512, periodic Hann, Slaney scale and norm) in device memory, four ways, run after run in turn: (a)
    pdmp3_amd_bulk_decode_clips_audio for the same spans; (b) (a) followed by torch.stft, abs() ** 2, a matmul with the
    filterbank and log10 (a dense matmul against the direct table where torch.stft cannot run); (c)
    pdmp3_amd_bulk_decode_clips_mel_long; (d) pdmp3_amd_bulk_decode_clips_stft_long(mode="power") followed by the matmul and
    log10 -- the route that writes the power batch to memory and reads it back.  (c) is compared once with (b) and (d)
    (largest difference, printed, not asserted: the tests check (c) against the definition).  Medians and min..max of --runs
    runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, n_fft, hop, n_mels, floor = args.clips, args.clip_frames, 44100, 2048, 512, 128, 1e-10
    bins = n_fft // 2 + 1
    sel = clip_selection(args, ixs, margin=2)
    Fm = (30 * rate) // hop if F == 1149 else (F * 1152 * rate // 44100) // hop
    T = (Fm - 1) * hop + n_fft
    dev = "cuda:0"
    mel, audio = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, n_fft // 2)                        # (no leading zeros: (a)'s rows start at start - n_fft / 2)
        mel.append((files[i], ixs[i], start))
        audio.append((files[i], ixs[i], start - n_fft // 2))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 1, n_mels, Fm), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, n_mels, Fm), dtype=torch.float32, device=dev)
    out_d = torch.zeros((K, 1, n_mels, Fm), dtype=torch.float32, device=dev)
    out_p = torch.zeros((K, 1, bins, Fm), dtype=torch.float32, device=dev)
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float32, device=dev)
    fb = torch.from_numpy(api.mel_long_filterbank(rate, n_fft, n_mels)).to(dev)                        # [n_mels, bins]
    kp = (bins + 15) // 16 * 16
    ang = 2.0 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(kp)[None, :]) % n_fft) / n_fft
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))[:, None]
    table = torch.from_numpy(np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1).astype(np.float32)).to(dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    how = {"stft": "torch.stft"}

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def torch_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)
        y = out_a[:, 0]
        p = None
        if how["stft"] == "torch.stft":
            try:
                p = torch.stft(y, n_fft, hop_length=hop, window=window, center=False, return_complex=True).abs() ** 2       # [K, bins, Fm]
            except Exception as e:                      # noqa: BLE001  (no FFT library on this build)
                how["stft"] = "dense matmul against the table (torch.stft: %s)" % type(e).__name__
        if p is None:
            x = y.unfold(1, n_fft, hop) @ table                                                                          # [K, Fm, 2 Kp]
            p = (x[:, :, :bins] ** 2 + x[:, :, kp:kp + bins] ** 2).transpose(1, 2)
        out_b[:, 0] = torch.log10(torch.clamp(torch.matmul(fb, p), min=floor))
        torch.cuda.synchronize()

    def mel_route():
        dec.decode_clips_mel_long(mel, Fm, rate, n_fft, hop, n_mels, floor=floor, out=out_c)

    def power_route():
        dec.decode_clips_stft_long(mel, Fm, rate, n_fft, hop, mode="power", out=out_p)
        out_d[:, 0] = torch.log10(torch.clamp(torch.matmul(fb, out_p[:, 0]), min=floor))
        torch.cuda.synchronize()

    routes = [("audio clips", audio_route), ("audio clips + torch.stft + matmul + log10", torch_route), ("mel_long clips", mel_route),
              ("stft_long power clips + matmul + log10", power_route)]
    diff = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: diff.update(
        {"torch_route": float((out_b - out_c).abs().max()), "power_route": float((out_d - out_c).abs().max())}))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as %d log10-mel bands x %d frames at %d Hz mono (n_fft %d, hop %d): %s" % (
               K, F, n_mels, Fm, rate, n_fft, hop, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "torch_route": how["stft"],
           "power_batch_bytes": K * bins * Fm * 4, "result_bytes": K * n_mels * Fm * 4,
           "largest_difference_from_mel_long": diff, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    res["mel_long_minus_audio_ms"] = round((med["mel_long clips"] - med["audio clips"]) * 1e3, 3)
    res["power_route_minus_audio_ms"] = round((med["stft_long power clips + matmul + log10"] - med["audio clips"]) * 1e3, 3)
    res["torch_route_minus_audio_ms"] = round((med["audio clips + torch.stft + matmul + log10"] - med["audio clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(spread * 1e3, 3)
    res["mel_long_cheaper_than_the_power_route_by_more_than_the_spread"] = bool(
        med["stft_long power clips + matmul + log10"] - med["mel_long clips"] > spread)
    close()
    print(json.dumps(res))


def clips_spectral(args, api):
    """--spectral: 64 clips of 30 s (--clips / --clip-frames change that) at 44.1 kHz mono as the six spectral descriptors x 2583
    frames (n_fft 2048, hop 512, periodic Hann; rms, zcr, centroid, bandwidth, roll-off 0.85, flatness) in device memory, four
    ways, run after run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the same spans; (b) (a) followed by torch.stft and the
    reductions in torch (a dense matmul against the direct table where torch.stft cannot run); (c)
    pdmp3_amd_bulk_decode_clips_spectral; (d) pdmp3_amd_bulk_decode_clips_stft_long(mode="magnitude") followed by the reductions
    of rows 2 .. 5 in torch -- the route that writes the magnitude batch to memory and reads it back (rows 0 and 1 need the signal,
    which (d) does not have: it computes four rows, and is the cheaper for it).  (c) is compared once with (b) and (d) (largest
    relative difference per row, printed, not asserted: the tests check (c) against the definition).  Medians and min..max of
    --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, n_fft, hop, roll, amin, zt = args.clips, args.clip_frames, 44100, 2048, 512, 0.85, 1e-10, 1e-10
    bins = n_fft // 2 + 1
    sel = clip_selection(args, ixs, margin=2)
    Fm = (30 * rate) // hop if F == 1149 else (F * 1152 * rate // 44100) // hop
    T = (Fm - 1) * hop + n_fft
    dev = "cuda:0"
    clips, audio = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, n_fft // 2)                        # (no leading zeros: (a)'s rows start at start - n_fft / 2)
        clips.append((files[i], ixs[i], start))
        audio.append((files[i], ixs[i], start - n_fft // 2))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 1, 6, Fm), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, 6, Fm), dtype=torch.float32, device=dev)
    out_d = torch.zeros((K, 1, 6, Fm), dtype=torch.float32, device=dev)
    out_s = torch.zeros((K, 1, bins, Fm), dtype=torch.float32, device=dev)
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float32, device=dev)
    freq = (torch.arange(bins, dtype=torch.float32, device=dev) * (rate / n_fft))[None, :, None]
    kp = (bins + 15) // 16 * 16
    ang = 2.0 * np.pi * ((np.arange(n_fft)[:, None] * np.arange(kp)[None, :]) % n_fft) / n_fft
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft))[:, None]
    table = torch.from_numpy(np.concatenate([w * np.cos(ang), -w * np.sin(ang)], axis=1).astype(np.float32)).to(dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    how = {"stft": "torch.stft"}

    def reductions(s, out):                              # s [K, bins, Fm] magnitudes -> rows 2 .. 5 of out [K, 6, Fm]
        total = s.sum(dim=1)
        safe = torch.clamp(total, min=1e-30)
        c = (freq * s).sum(dim=1) / safe
        out[:, 2] = c
        out[:, 3] = torch.sqrt((s * (freq - c[:, None, :]) ** 2).sum(dim=1) / safe)
        k = (torch.cumsum(s, dim=1) < (roll * total)[:, None, :]).sum(dim=1)
        out[:, 4] = torch.clamp(k, max=bins - 1).to(torch.float32) * (rate / n_fft)
        pm = torch.clamp(s * s, min=amin)
        out[:, 5] = torch.exp(torch.log(pm).mean(dim=1)) / pm.mean(dim=1)

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def torch_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)
        y = out_a[:, 0]
        s = None
        if how["stft"] == "torch.stft":
            try:
                s = torch.stft(y, n_fft, hop_length=hop, window=window, center=False, return_complex=True).abs()            # [K, bins, Fm]
            except Exception as e:                      # noqa: BLE001  (no FFT library on this build)
                how["stft"] = "dense matmul against the table (torch.stft: %s)" % type(e).__name__
        fr = y.unfold(1, n_fft, hop)                                                                                      # [K, Fm, N]
        if s is None:
            x = fr @ table                                                                                                # [K, Fm, 2 Kp]
            s = torch.sqrt(x[:, :, :bins] ** 2 + x[:, :, kp:kp + bins] ** 2).transpose(1, 2)
        out_b[:, 0, 0] = torch.sqrt((fr * fr).mean(dim=2))
        neg = fr < -zt
        out_b[:, 0, 1] = (neg[:, :, 1:] != neg[:, :, :-1]).sum(dim=2).to(torch.float32) / n_fft
        reductions(s, out_b[:, 0])
        torch.cuda.synchronize()

    def spectral_route():
        dec.decode_clips_spectral(clips, Fm, rate, n_fft, hop, roll, amin, zt, channels=1, out=out_c)

    def magnitude_route():
        dec.decode_clips_stft_long(clips, Fm, rate, n_fft, hop, mode="magnitude", out=out_s)
        reductions(out_s[:, 0], out_d[:, 0])
        torch.cuda.synchronize()

    routes = [("audio clips", audio_route), ("audio clips + torch.stft + reductions", torch_route), ("spectral clips", spectral_route),
              ("stft_long magnitude clips + reductions", magnitude_route)]
    rel = lambda o, rows: [float(((o[:, 0, i] - out_c[:, 0, i]).abs() / torch.clamp(out_c[:, 0, i].abs(), min=1e-3)).max()) for i in rows]
    diff = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: diff.update(
        {"torch_route_rows_0_to_5": rel(out_b, range(6)), "magnitude_route_rows_2_to_5": rel(out_d, range(2, 6))}))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as 6 spectral descriptors x %d frames at %d Hz mono (n_fft %d, hop %d): %s" % (
               K, F, Fm, rate, n_fft, hop, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "torch_route": how["stft"],
           "magnitude_batch_bytes": K * bins * Fm * 4, "result_bytes": K * 6 * Fm * 4,
           "largest_relative_difference_from_spectral": diff, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    res["spectral_minus_audio_ms"] = round((med["spectral clips"] - med["audio clips"]) * 1e3, 3)
    res["magnitude_route_minus_audio_ms"] = round((med["stft_long magnitude clips + reductions"] - med["audio clips"]) * 1e3, 3)
    res["torch_route_minus_audio_ms"] = round((med["audio clips + torch.stft + reductions"] - med["audio clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(spread * 1e3, 3)
    res["spectral_cheaper_than_the_magnitude_route_by_more_than_the_spread"] = bool(
        med["stft_long magnitude clips + reductions"] - med["spectral clips"] > spread)
    res["spectral_cheaper_than_the_torch_route_by_more_than_the_spread"] = bool(
        med["audio clips + torch.stft + reductions"] - med["spectral clips"] > spread)
    close()
    print(json.dumps(res))


def clips_hpss(args, api):
    """--hpss: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono as the soft masks of median-filter
    harmonic-percussive separation [2, 1025, 1292] (n_fft 2048, hop 512, kernels 31 / 31, power 2, margins 1) in device memory,
    four ways, run after run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the widened spans; (b)
    pdmp3_amd_bulk_decode_clips_stft_long(mode="magnitude") of the widened clips; (c) pdmp3_amd_bulk_decode_clips_hpss; (d) (b)
    followed by the same algorithm in torch -- unfold + median along both axes, then the mask.  (c) is compared once with (d)
    (largest difference, printed, not asserted: the tests check (c) against the definition).  Also timed with device events: a
    plain copy of two planes, the bytes k_clip_hpss writes.  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, n_fft, hop, lh, lp = args.clips, args.clip_frames, 22050, 2048, 512, 31, 31
    bins, rh, rp = n_fft // 2 + 1, lh // 2, lp // 2
    sel = clip_selection(args, ixs, margin=2)
    Fm = (30 * rate) // hop if F == 1149 else (F * 1152 * rate // 44100) // hop
    Fw = Fm + 2 * rh
    T = (Fw - 1) * hop + n_fft
    dev = "cuda:0"
    clips, wide, audio = [], [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, n_fft // 2 + rh * hop)                       # (no leading zeros in the widened clip)
        clips.append((files[i], ixs[i], start))
        wide.append((files[i], ixs[i], start - rh * hop))
        audio.append((files[i], ixs[i], start - rh * hop - n_fft // 2))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_s = torch.zeros((K, 1, bins, Fw), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, 2, bins, Fm), dtype=torch.float32, device=dev)
    out_d = torch.zeros((K, 1, 2, bins, Fm), dtype=torch.float32, device=dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def magnitude_route():
        dec.decode_clips_stft_long(wide, Fw, rate, n_fft, hop, mode="magnitude", out=out_s)

    def hpss_route():
        dec.decode_clips_hpss(clips, Fm, rate, n_fft, hop, (lh, lp), 2.0, 1.0, "mask", channels=1, out=out_c)

    def torch_route():
        dec.decode_clips_stft_long(wide, Fw, rate, n_fft, hop, mode="magnitude", out=out_s)
        for k in range(K):                               # (a clip at a time: the unfolded windows of one are 31 x its spectrogram)
            s = out_s[k, 0]                                                                   # [bins, Fw]
            hm = s.unfold(1, lh, 1).median(dim=2).values                                      # [bins, Fm]
            c = s[:, rh:rh + Fm]
            sym = torch.cat([c[:rp].flip(0), c, c[bins - rp:].flip(0)], dim=0)                # numpy's "symmetric"
            pm = sym.unfold(0, lp, 1).median(dim=2).values                                    # [bins, Fm]
            h2, p2 = hm.double() ** 2, pm.double() ** 2
            tot = h2 + p2
            silent = torch.maximum(hm, pm) < 2.0 ** -126
            safe = torch.where(silent, torch.ones_like(tot), tot)
            out_d[k, 0, 0] = torch.where(silent, 0.5, h2 / safe).float()
            out_d[k, 0, 1] = torch.where(silent, 0.5, p2 / safe).float()
        torch.cuda.synchronize()

    routes = [("audio clips", audio_route), ("stft_long magnitude clips", magnitude_route), ("hpss clips", hpss_route),
              ("stft_long magnitude clips + torch medians and masks", torch_route)]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(diff=float((out_d - out_c).abs().max())))
    copies = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(args.warmup_runs + args.runs):
        e0.record()
        out_d.copy_(out_c)
        e1.record()
        torch.cuda.synchronize()
        if r >= args.warmup_runs:
            copies.append(e0.elapsed_time(e1))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as harmonic and percussive masks [2, %d, %d] at %d Hz mono (n_fft %d, hop %d, kernels %d / %d, "
                       "power 2): %s" % (K, F, bins, Fm, rate, n_fft, hop, lh, lp,
                                         corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "stage_bytes": K * bins * Fw * 4, "result_bytes": K * 2 * bins * Fm * 4, "largest_difference_of_the_torch_route_from_hpss": seen["diff"],
           "plain_copy_of_the_result_ms": {"median": round(statistics.median(copies), 4), "min": round(min(copies), 4), "max": round(max(copies), 4)},
           "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    res["hpss_minus_magnitude_ms"] = round((med["hpss clips"] - med["stft_long magnitude clips"]) * 1e3, 3)
    res["torch_route_minus_magnitude_ms"] = round((med["stft_long magnitude clips + torch medians and masks"] - med["stft_long magnitude clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(spread * 1e3, 3)
    res["hpss_cheaper_than_the_torch_route_by_more_than_the_spread"] = bool(
        med["stft_long magnitude clips + torch medians and masks"] - med["hpss clips"] > spread)
    close()
    print(json.dumps(res))


def clips_mfcc_long(args, api):
    """--mfcc-long: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono as librosa's MFCC with both deltas
    [60, 1292] (n_fft 2048, hop 512, 128 bands, 20 cepstra, top_db 80, delta width 9) in device memory, three ways, run after run
    in turn: (a) pdmp3_amd_bulk_decode_clips_mel_long (log10) of the widened clips alone; (b) pdmp3_amd_bulk_decode_clips_mfcc_long;
    (c) (a) followed by the same chain in torch -- amax, clamp, matmul, conv1d.  (b) is compared once with (c) (largest
    difference, printed, not asserted: the tests check (b) against the definition).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, n_fft, hop, nm, nc, w, top = args.clips, args.clip_frames, 22050, 2048, 512, 128, 20, 9, 80.0
    h = (w - 1) // 2
    sel = clip_selection(args, ixs, margin=2)
    Fm = (30 * rate) // hop if F == 1149 else (F * 1152 * rate // 44100) // hop
    Fw = Fm + 2 * h
    dev = "cuda:0"
    clips, wide = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, n_fft // 2 + h * hop)
        clips.append((files[i], ixs[i], start))
        wide.append((files[i], ixs[i], start - h * hop))
    out_l = torch.zeros((K, 1, nm, Fw), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 1, 3 * nc, Fm), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, 3 * nc, Fm), dtype=torch.float32, device=dev)
    table = torch.from_numpy(api.mfcc_long_dct_table(nm, nc, 0.0)[:nc, :nm].copy()).to(dev)
    taps = torch.from_numpy(api.mfcc_long_delta_taps(w).astype(np.float32)).to(dev).reshape(2, 1, w)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def mel_route():
        dec.decode_clips_mel_long(wide, Fw, rate, n_fft, hop, nm, mode="log10", floor=1e-10, out=out_l)

    def mfcc_route():
        dec.decode_clips_mfcc_long(clips, Fm, rate, n_fft, hop, nm, nc, 0.0, top, 1e-10, 2, w, "mfcc", out=out_b)

    def torch_route():
        dec.decode_clips_mel_long(wide, Fw, rate, n_fft, hop, nm, mode="log10", floor=1e-10, out=out_l)
        d = out_l[:, 0] * 10.0                                                            # [K, nm, Fw]
        d = torch.maximum(d, d[:, :, h:h + Fm].amax(dim=(1, 2), keepdim=True) - top)
        c = torch.matmul(table, d)                                                        # [K, nc, Fw]
        dl = torch.nn.functional.conv1d(c.reshape(K * nc, 1, Fw), taps).reshape(K, nc, 2, Fm)
        out_c[:, 0, :nc] = c[:, :, h:h + Fm]
        out_c[:, 0, nc:2 * nc] = dl[:, :, 0]
        out_c[:, 0, 2 * nc:] = dl[:, :, 1]
        torch.cuda.synchronize()

    routes = [("mel_long log10 clips", mel_route), ("mfcc_long clips", mfcc_route), ("mel_long log10 clips + torch amax, clamp, matmul, conv1d", torch_route)]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(diff=float((out_c - out_b).abs().max())))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as MFCC, delta and delta-delta [%d, %d] at %d Hz mono (n_fft %d, hop %d, %d bands, %d cepstra, "
                       "top_db %g, width %d): %s" % (K, F, 3 * nc, Fm, rate, n_fft, hop, nm, nc, top, w,
                                                     corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "stage_bytes": K * nm * Fw * 4, "result_bytes": K * 3 * nc * Fm * 4, "largest_difference_of_the_torch_route_from_mfcc_long": seen["diff"],
           "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    spread = max(max(ts) - min(ts) for ts in times.values())
    res["mfcc_long_minus_mel_long_ms"] = round((med["mfcc_long clips"] - med["mel_long log10 clips"]) * 1e3, 3)
    res["torch_route_minus_mel_long_ms"] = round((med[routes[2][0]] - med["mel_long log10 clips"]) * 1e3, 3)
    res["mfcc_long_over_mel_long"] = round(med["mfcc_long clips"] / med["mel_long log10 clips"], 4)
    res["largest_spread_ms"] = round(spread * 1e3, 3)
    res["mfcc_long_cheaper_than_the_torch_route_by_more_than_the_spread"] = bool(med[routes[2][0]] - med["mfcc_long clips"] > spread)
    close()
    print(json.dumps(res))


def clips_cqt(args, api):
    """--cqt: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono as the magnitudes of 84 constant-Q bins
    (C1, 12 an octave, norm 1, scale 1) x 1292 frames (hop 512) in device memory, three ways, run after run in turn: (a)
    pdmp3_amd_bulk_decode_clips_audio for the same spans; (b) (a) followed by a dense torch matmul of the unfolded frames with
    the table as a dense [N_0, 2 x 84] matrix (every bin at the longest filter's length), eight clips at a time, and the
    magnitude; (c) pdmp3_amd_bulk_decode_clips_cqt.  (c) is compared once with (b) (largest difference, printed, not asserted:
    the tests check (c) against the definition).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, hop, n_bins = args.clips, args.clip_frames, 22050, 512, 84
    f_k, half = api.cqt_lengths(rate)
    h0 = int(half[0])
    n0 = 2 * h0 + 1
    sel = clip_selection(args, ixs, margin=2)
    Fm = 1292 if F == 1149 else (F * 1152 * rate // 44100) // hop + 1
    T = (Fm - 1) * hop + n0
    dev = "cuda:0"
    cq, audio = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, h0)                                # (no leading zeros: (a)'s rows start at start - h_0)
        cq.append((files[i], ixs[i], start))
        audio.append((files[i], ixs[i], start - h0))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 1, n_bins, Fm), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, n_bins, Fm), dtype=torch.float32, device=dev)
    tab, rows, at = api.cqt_table(rate)
    dense = np.zeros((n0, 2 * n_bins), dtype=np.float32)
    for k in range(n_bins):
        t = k // 16
        r0, n = h0 - int(half[16 * t]), min(int(rows[t]), n0 - (h0 - int(half[16 * t])))
        dense[r0:r0 + n, k] = tab[at[t]:at[t] + n, k % 16]
        dense[r0:r0 + n, n_bins + k] = tab[at[t]:at[t] + n, 16 + k % 16]
    dense = torch.from_numpy(dense).to(dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def torch_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)
        for k0 in range(0, K, 8):
            x = out_a[k0:k0 + 8, 0].unfold(1, n0, hop) @ dense                                                           # [8, Fm, 2 x 84]
            out_b[k0:k0 + 8, 0] = torch.sqrt(x[:, :, :n_bins] ** 2 + x[:, :, n_bins:] ** 2).transpose(1, 2)
        torch.cuda.synchronize()

    def cqt_route():
        dec.decode_clips_cqt(cq, Fm, rate, hop, out=out_c)

    routes = [("audio clips", audio_route), ("audio clips + dense torch matmul + magnitude", torch_route), ("cqt clips", cqt_route)]
    diff = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: diff.update(
        {"torch_route": float((out_b - out_c).abs().max()), "largest_magnitude": float(out_c.abs().max())}))
    dec.close()
    plan = api.cqt_plan(rate, hop=hop)
    res = {"workload": "%d clips of %d frames' length as %d constant-Q bins x %d frames at %d Hz mono (C1, 12 an octave, hop %d): %s" % (
               K, F, n_bins, Fm, rate, hop, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "plan": {"tile": plan[0], "lds_bytes": plan[2], "split_tiles": plan[5], "table_rows": int(rows.sum()), "dense_rows": 6 * int(rows[0])},
           "result_bytes": K * n_bins * Fm * 4, "largest_difference_from_cqt": diff, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    res["cqt_minus_audio_ms"] = round((med["cqt clips"] - med["audio clips"]) * 1e3, 3)
    res["torch_route_minus_audio_ms"] = round((med["audio clips + dense torch matmul + magnitude"] - med["audio clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def clips_chroma(args, api):
    """--chroma: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono as 12 pitch classes x 1292 frames (the
    default spec: C1, 84 bins, 12 an octave, hop 512, magnitudes, max norm) in device memory, three ways, run after run in turn:
    (a) pdmp3_amd_bulk_decode_clips_audio for the same spans; (b) pdmp3_amd_bulk_decode_clips_cqt's magnitudes [K, 1, 84, F]
    folded over the seven octaves and divided by the frame's maximum in torch; (c) pdmp3_amd_bulk_decode_clips_chroma.  (c) is
    compared once with (b) (largest difference, printed, not asserted: torch adds the octaves in its own order, and the tests
    check (c) against the definition and against the sequential fold).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, hop, n_bins, n_chroma, floor = args.clips, args.clip_frames, 22050, 512, 84, 12, 1e-10
    h0 = int(api.cqt_lengths(rate)[1][0])
    n0 = 2 * h0 + 1
    sel = clip_selection(args, ixs, margin=2)
    Fm = 1292 if F == 1149 else (F * 1152 * rate // 44100) // hop + 1
    T = (Fm - 1) * hop + n0
    dev = "cuda:0"
    cq, audio = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate, h0)                                # (no leading zeros: (a)'s rows start at start - h_0)
        cq.append((files[i], ixs[i], start))
        audio.append((files[i], ixs[i], start - h0))
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_q = torch.zeros((K, 1, n_bins, Fm), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 1, n_chroma, Fm), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, n_chroma, Fm), dtype=torch.float32, device=dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(audio, T, rate, 1, out=out_a)

    def cqt_route():
        dec.decode_clips_cqt(cq, Fm, rate, hop, out=out_q)
        c = out_q.view(K, 1, n_bins // n_chroma, n_chroma, Fm).sum(dim=2)
        torch.div(c, c.amax(dim=2, keepdim=True).clamp_min(floor), out=out_b)
        torch.cuda.synchronize()

    def chroma_route():
        dec.decode_clips_chroma(cq, Fm, rate, hop, channels=1, norm_floor=floor, out=out_c)

    routes = [("audio clips", audio_route), ("cqt clips + fold + max norm in torch", cqt_route), ("chroma clips", chroma_route)]
    diff = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: diff.update(
        {"torch_route": float((out_b - out_c).abs().max()), "largest_value": float(out_c.abs().max()),
         "frames_at_one": int((out_c.amax(dim=2) == 1.0).sum()), "frames": K * Fm}))
    dec.close()
    plan = api.chroma_plan(rate, hop=hop)
    res = {"workload": "%d clips of %d frames' length as %d pitch classes x %d frames at %d Hz mono (C1, %d bins, 12 an octave, hop %d): %s" % (
               K, F, n_chroma, Fm, rate, n_bins, hop, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "plan": {"tile": plan[0], "lds_bytes": plan[2], "split_tiles": plan[5]},
           "result_bytes": K * n_chroma * Fm * 4, "cqt_bytes": K * n_bins * Fm * 4, "largest_difference_from_chroma": diff, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    res["chroma_minus_audio_ms"] = round((med["chroma clips"] - med["audio clips"]) * 1e3, 3)
    res["cqt_route_minus_audio_ms"] = round((med["cqt clips + fold + max norm in torch"] - med["audio clips"]) * 1e3, 3)
    res["chroma_minus_cqt_route_ms"] = round((med["chroma clips"] - med["cqt clips + fold + max norm in torch"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def clips_loudness(args, api, r128=False):
    """--r128: --loudness's batch and routes with a third one in the rotation, (c) pdmp3_amd_bulk_decode_clips_r128 for the same
    clips with the same target under -1 dBTP (audio times the gain, stats of 16, no curves): true peak, short-term loudness
    and loudness range on top of (b).  (c) minus (b) is reported, not capped (profiles/clip_r128.txt).
    --loudness: 64 clips of 30 s (--clips / --clip-frames change that) at 32 000 Hz stereo in device memory, two ways, run after
    run in turn: (a) pdmp3_amd_bulk_decode_clips_audio; (b) pdmp3_amd_bulk_decode_clips_loudness for the same clips with target
    -14 LUFS (audio times the gain, stats, no momentary curve).  There is no torch route to hold against: torch without
    torchaudio has no recursive filter.  (b) minus (a) is reported, not capped.  The kernels' own times come from a
    kernel-trace run of this mode (profiles/clip_loudness.txt).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, target = args.clips, args.clip_frames, 32000, -14.0
    T = 30 * rate if F == 1149 else F * 1152 * rate // 44100
    sel = clip_selection(args, ixs, margin=2)
    clips = [(files[i], ixs[i], clip_start(ixs[i], a, rate)) for i, a in sel]
    dev = "cuda:0"
    out_a = torch.zeros((K, 2, T), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 2, T), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 2, T), dtype=torch.float32, device=dev) if r128 else None
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    stats = [None, None]

    def audio_route():
        dec.decode_clips_audio(clips, T, rate, 2, out=out_a)

    def loudness_route():
        stats[0] = dec.decode_clips_loudness(clips, T, rate, 2, target=target, out=out_b)[1]

    def r128_route():
        stats[1] = dec.decode_clips_r128(clips, T, rate, 2, target=target, out=out_c)[1]

    routes = [("audio clips", audio_route), ("loudness clips", loudness_route)] + ([("r128 clips", r128_route)] if r128 else [])
    seen = {}

    def compare():
        st = stats[0].cpu().numpy()
        fin = np.isfinite(st[:, 0])
        seen.update({"audio_is_x_times_g": bool(torch.equal(out_b, out_a * stats[0][:, 3].view(K, 1, 1))), "clips_with_a_loudness": int(fin.sum()),
                     "L_min": float(st[fin, 0].min()) if fin.any() else None, "L_max": float(st[fin, 0].max()) if fin.any() else None,
                     "g_min": float(st[:, 3].min()), "g_max": float(st[:, 3].max()), "blocks": int(st[0, 5])})
        if r128:
            sr = stats[1].cpu().numpy()
            seen.update({"r128_audio_is_x_times_g": bool(torch.equal(out_c, out_a * stats[1][:, 3].view(K, 1, 1))),
                         "r128_first_three_are_the_loudness_calls": bool((sr[:, :3].view(np.uint32) == st[:, :3].view(np.uint32)).all()),
                         "clips_held_to_the_true_peak": int((sr[:, 3] < st[:, 3]).sum()), "TP_over_P_max": float((sr[:, 8] / np.maximum(sr[:, 2], 1e-30)).max()),
                         "TP_max": float(sr[:, 8].max()), "LRA_min": float(sr[:, 10].min()), "LRA_max": float(sr[:, 10].max()),
                         "windows": int(sr[0, 12]), "range_windows": int(sr[0, 13])})
    times = time_routes(routes, args.warmup_runs, args.runs, compare)
    dec.close()
    plan = api.loudness_plan(rate, T)
    res = {"workload": "%d clips of %d samples at %d Hz stereo, K-weighted, gated and scaled to %g LUFS: %s" % (
               K, T, rate, target, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "plan": {"block": plan[0], "chunk_blocks": plan[1], "lds_bytes": plan[2], "q": plan[3], "chunks": plan[4], "I": plan[5], "J": plan[6]},
           "batch_bytes": K * 2 * T * 4, "seen": seen, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    res["loudness_minus_audio_ms"] = round((med["loudness clips"] - med["audio clips"]) * 1e3, 3)
    if r128:
        res["r128_minus_loudness_ms"] = round((med["r128 clips"] - med["loudness clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def torch_yin(x, rate, N, W, H, tmin, tmax, thr):
    """YIN as include/pdmp3_bulk.h defines it (items 3-6), for rows x [K, T] whose first sample is the first frame's first, with
    torch's own kernels in binary32 -> [K, 3, F]: f0, d'(tau*), tau*"""
    import torch
    lag = torch.arange(tmax + 1, dtype=torch.float32, device=x.device)
    fr = x.unfold(-1, N, H)                                        # [K, F, N]
    r = torch.fft.irfft(torch.fft.rfft(fr, n=N) * torch.fft.rfft(fr[..., :W], n=N).conj(), n=N)[..., :tmax + 1]
    cs = torch.nn.functional.pad(torch.cumsum(fr * fr, -1), (1, 0))
    e = cs[..., W:W + tmax + 1] - cs[..., :tmax + 1]
    d = e[..., :1] + e - 2.0 * r
    S = torch.cumsum(d[..., 1:], -1)
    dp = torch.ones_like(d)
    dp[..., 1:] = torch.where(S > 0, d[..., 1:] * lag[1:] / S, torch.ones_like(S))
    c = dp[..., tmin:tmax + 1]
    trough = torch.zeros_like(c, dtype=torch.bool)
    trough[..., 1:-1] = (c[..., 1:-1] < c[..., :-2]) & (c[..., 1:-1] <= c[..., 2:])
    trough[..., 0] = c[..., 0] < c[..., 1]
    under = trough & (c < thr)
    first = torch.argmax(under.to(torch.int8), -1)
    best = torch.where(under.any(-1), first, torch.argmin(c, -1))
    i0 = best.unsqueeze(-1)
    b = torch.gather(c, -1, i0)
    a = torch.gather(c, -1, (i0 - 1).clamp(min=0))
    cc = torch.gather(c, -1, (i0 + 1).clamp(max=tmax - tmin))
    D = a - 2.0 * b + cc
    inner = (i0 > 0) & (i0 < tmax - tmin) & (D > 0)
    delta = torch.where(inner, (a - cc) / (2.0 * torch.where(inner, D, torch.ones_like(D))), torch.zeros_like(D))
    tau = (best + tmin).to(torch.float32)
    silent = ~(fr != 0).any(-1)
    return torch.stack([torch.where(silent, torch.zeros_like(tau), rate / (tau + delta.squeeze(-1))),
                        torch.where(silent, torch.ones_like(tau), b.squeeze(-1)), torch.where(silent, torch.zeros_like(tau), tau)], 1)


def clips_pitch(args, api):
    """--pitch: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono as YIN pitch [K, 1, 3, 1292] with
    librosa.yin's defaults (frame 2048, window 1024, hop 512, C2 .. C7, threshold 0.1) in device memory, three ways, run after
    run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the same spans (the call the feature call makes itself); (b) (a)
    followed by the same algorithm in torch on the device -- unfold, torch.fft.rfft / irfft for r, cumulative sums for e and S,
    the decision with argmax / argmin, the parabola --; (c) pdmp3_amd_bulk_decode_clips_pitch.  (b) and (c) are compared once
    (share of frames with the same lag and the largest f0 difference among them, printed, not asserted: the tests check (c)
    against the definition).  k_clip_pitch's own time comes from a kernel-trace run of this mode (profiles/clip_pitch.txt).
    Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, Fm, rate, N, W, H, thr = args.clips, args.clip_frames, 22050, 2048, 1024, 512, 0.1
    span = 30 * rate if Fm == 1149 else Fm * 1152 * rate // 44100
    F = span // H + 1
    T = (F - 1) * H + N
    tmin, tmax, tiles = api.pitch_lags(rate)
    sel = clip_selection(args, ixs, first=2, margin=4)
    clips, spans = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate)
        clips.append((files[i], ixs[i], start))
        spans.append((files[i], ixs[i], start - N // 2))
    dev = "cuda:0"
    sig = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_b = torch.zeros((K, 1, 3, F), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, 3, F), dtype=torch.float32, device=dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(spans, T, rate, 1, out=sig)

    def torch_route():
        dec.decode_clips_audio(spans, T, rate, 1, out=sig)
        out_b[:, 0] = torch_yin(sig[:, 0], rate, N, W, H, tmin, tmax, thr)
        torch.cuda.synchronize()

    def pitch_route():
        dec.decode_clips_pitch(clips, F, rate, N, H, out=out_c)

    routes = [("audio clips", audio_route), ("audio clips + torch yin", torch_route), ("pitch clips", pitch_route)]
    seen = {}

    def compare():
        same = out_b[:, 0, 2] == out_c[:, 0, 2]
        seen.update({"frames": int(same.numel()), "frames_with_torchs_lag": int(same.sum()),
                     "largest_f0_difference_among_them_hz": float((out_b[:, 0, 0] - out_c[:, 0, 0])[same].abs().max()) if bool(same.any()) else None,
                     "voiced_frames": int((out_c[:, 0, 1] < thr).sum()), "frames_of_zeros": int((out_c[:, 0, 2] == 0).sum())})
    times = time_routes(routes, args.warmup_runs, args.runs, compare)
    dec.close()
    plan = api.pitch_plan(rate)
    res = {"workload": "%d clips of %d frames (%d samples) at %d Hz mono, YIN, frame %d window %d hop %d, lags %d .. %d: %s" % (
               K, F, T, rate, N, W, H, tmin, tmax, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "plan": {"frames_a_workgroup": plan[0], "span_floats": plan[1], "lds_bytes": plan[2], "matrix_instructions_a_tile": plan[3], "lag_tiles": tiles},
           "matrix_instructions": K * F * tiles * plan[3], "seen": seen, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    res["pitch_minus_audio_ms"] = round((med["pitch clips"] - med["audio clips"]) * 1e3, 3)
    res["torch_minus_audio_ms"] = round((med["audio clips + torch yin"] - med["audio clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def clips_pyin(args, api):
    """--pyin: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono through pYIN with librosa.pyin's defaults
    (frame 2048, window 1024, hop 512, C2 .. C7, 100 thresholds, 601 bins, a band of 101) in device memory, four ways, run after
    run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the same spans; (b) pdmp3_amd_bulk_decode_clips_pitch's curve
    [K, 1, 339, F], which a caller without this call takes off the device; (c) pdmp3_amd_bulk_decode_clips_pyin's observation
    [K, 1, 602, F]; (d) its path [K, 1, 4, F].  The kernels' own times come from a kernel-trace run of this mode
    (profiles/clip_pyin.txt).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, Fm, rate, N, H = args.clips, args.clip_frames, 22050, 2048, 512
    span = 30 * rate if Fm == 1149 else Fm * 1152 * rate // 44100
    F = span // H + 1
    T = (F - 1) * H + N
    tmin, tmax, _ = api.pitch_lags(rate)
    plan = api.pyin_plan(rate, n_frames=F)
    sel = clip_selection(args, ixs, first=2, margin=4)
    clips, spans = [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate)
        clips.append((files[i], ixs[i], start))
        spans.append((files[i], ixs[i], start - N // 2))
    dev = "cuda:0"
    sig = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    curve = torch.zeros((K, 1, tmax + 1, F), dtype=torch.float32, device=dev)
    obs = torch.zeros((K, 1, plan["n_bins"] + 1, F), dtype=torch.float32, device=dev)
    path = torch.zeros((K, 1, 4, F), dtype=torch.float32, device=dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    routes = [("audio clips", lambda: dec.decode_clips_audio(spans, T, rate, 1, out=sig)),
              ("pitch curve clips", lambda: dec.decode_clips_pitch(clips, F, rate, N, H, out_mode="curve", out=curve)),
              ("pyin observation clips", lambda: dec.decode_clips_pyin(clips, F, rate, 1, out_mode="observation", out=obs)),
              ("pyin path clips", lambda: dec.decode_clips_pyin(clips, F, rate, 1, out=path))]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(
        {"frames": K * F, "voiced_frames": int((path[:, 0, 1] == 1).sum()), "mean_voiced_probability": float(path[:, 0, 2].mean()),
         "non_zero_observations_a_frame": float((obs[:, 0, :-1] != 0).sum()) / (K * F),
         "path_v_is_observation_v": bool(torch.equal(path[:, 0, 2], obs[:, 0, -1]))}))
    dec.close()
    res = {"workload": "%d clips of %d frames (%d samples) at %d Hz mono, pYIN, frame %d hop %d, lags %d .. %d, %d bins, band %d: %s" % (
               K, F, T, rate, N, H, tmin, tmax, plan["n_bins"], plan["band"], corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "plan": plan,
           "curve_batch_bytes": int(curve.numel() * 4), "stage_bytes": K * (plan["curve_bytes"] + plan["obs_bytes"] + plan["bp_bytes"]),
           "seen": seen, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    res["observation_minus_curve_ms"] = round((med["pyin observation clips"] - med["pitch curve clips"]) * 1e3, 3)
    res["path_minus_curve_ms"] = round((med["pyin path clips"] - med["pitch curve clips"]) * 1e3, 3)
    res["path_minus_audio_ms"] = round((med["pyin path clips"] - med["audio clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def clips_beat(args, api):
    """--beat: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono through the beat tracker with librosa's
    defaults (n_fft 2048, hop 512, 128 bands, tempogram window 384, tightness 100, trim) in device memory, run after run in turn:
    (a) pdmp3_amd_bulk_decode_clips_tempogram in mode "onset"; (b) the same call in mode "tempo"; (c) pdmp3_amd_bulk_decode_clips_beats
    with the tempo estimated; (d) with bpm 120 given.  Beside the rotation, twice: (e) mode "onset", a copy to the host and the
    numpy restatement of the tracker (tests/clip_beat_ref.py) clip by clip at the period (b) decided -- what a caller without this
    call does.  The kernels' own times come from a kernel-trace run of this mode (profiles/clip_beat.txt).  Medians and min..max
    of --runs runs."""
    import torch
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import clip_beat_ref as ref
    files, ixs, close = clip_corpus(args, api)
    K, Fm, rate, N, H = args.clips, args.clip_frames, 22050, 2048, 512
    span = 30 * rate if Fm == 1149 else Fm * 1152 * rate // 44100
    F = span // H + 1
    plan_est, plan_given = api.beat_plan(rate, n_frames=F), api.beat_plan(rate, n_frames=F, bpm=120.0)
    clips = [(files[i], ixs[i], clip_start(ixs[i], a, rate)) for i, a in clip_selection(args, ixs, first=200, margin=200)]
    dev = "cuda:0"
    onset = torch.zeros((K, 1, F), dtype=torch.float32, device=dev)
    tempo = torch.zeros((K, 1, 4), dtype=torch.float32, device=dev)
    beats = torch.zeros((K, 1, 2, F), dtype=torch.float32, device=dev)
    given = torch.zeros((K, 1, 2, F), dtype=torch.float32, device=dev)
    stats = torch.zeros((K, 1, 8), dtype=torch.float32, device=dev)
    stats_g = torch.zeros((K, 1, 8), dtype=torch.float32, device=dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    routes = [("tempogram clips, onset", lambda: dec.decode_clips_tempogram(clips, F, rate, out_mode="onset", out=onset)),
              ("tempogram clips, tempo", lambda: dec.decode_clips_tempogram(clips, F, rate, out_mode="tempo", out=tempo)),
              ("beat clips, tempo estimated", lambda: dec.decode_clips_beats(clips, F, rate, out=beats, stats=stats)),
              ("beat clips, bpm 120", lambda: dec.decode_clips_beats(clips, F, rate, bpm=120.0, out=given, stats=stats_g))]
    times = time_routes(routes, args.warmup_runs, args.runs)
    periods = [int(x) for x in tempo[:, 0, 1].cpu().numpy()]
    tabs = {p: api.beat_tables(p) for p in set(periods)}
    host_times, same = [], True
    for r in range(2):
        t0 = time.perf_counter()
        dec.decode_clips_tempogram(clips, F, rate, out_mode="onset", out=onset)
        o = onset.cpu().numpy()
        rows = [ref.track(o[k, 0], F, periods[k], tabs[periods[k]][0], tabs[periods[k]][1], True)["beats"] for k in range(K)]
        host_times.append(time.perf_counter() - t0)
        same = same and bool(np.array_equal(np.stack(rows), beats[:, 0].cpu().numpy()))
    dec.close()
    st = stats[:, 0].cpu().numpy()
    res = {"workload": "%d clips of %d frames at %d Hz mono, beat tracking, n_fft %d hop %d, tightness 100, trim: %s" % (
               K, F, rate, N, H, corpus_name(args, files)),
           "source_rates": sorted(set(ix.rate for _, ix, _ in clips)), "destination": "device memory", "runs": args.runs,
           "plan_estimated": plan_est, "plan_bpm_120": plan_given,
           "seen": {"periods": sorted(set(periods)), "beats_kept_mean": float(st[:, 2].mean()), "beats_before_trim_mean": float(st[:, 3].mean()),
                    "device_is_the_numpy_restatement": same},
           "onset + copy + numpy restatement": {"seconds": {"min": round(min(host_times), 6), "max": round(max(host_times), 6)}},
           "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    res["estimated_minus_tempo_ms"] = round((med["beat clips, tempo estimated"] - med["tempogram clips, tempo"]) * 1e3, 3)
    res["bpm_120_minus_onset_ms"] = round((med["beat clips, bpm 120"] - med["tempogram clips, onset"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def torch_tempogram(l, lag, wt, f, window, prior, rate, hop, mode):
    """the definition of DESIGN.md section 21 (max_size 1) in torch on the device: l [K, n_mels, n_env + lag] log10 mel ->
    mode 0 [K, n_env], 1 [K, wt, f], 2 [K, 4]"""
    import torch
    o = 10.0 * torch.relu(l[..., lag:] - l[..., :-lag]).mean(dim=1)
    if mode == 0:
        return o
    x = o.unfold(-1, wt, 1) * window                                            # [K, f, wt]
    r = torch.fft.irfft(torch.fft.rfft(x, 2 * wt).abs() ** 2, 2 * wt)[..., :wt]
    r0 = r[..., :1]
    t = torch.where(r0 > 0, r / r0.clamp_min(1e-30), torch.zeros_like(r)).transpose(1, 2)
    if mode == 1:
        return t
    s = torch.log1p(1e6 * t.to(torch.float64).mean(-1).clamp_min(0.0)) + prior
    top = torch.topk(s, 2, dim=-1)
    tau = top.indices[:, 0].to(torch.float64)
    return torch.stack([60.0 * rate / (hop * tau), tau, top.values[:, 0], top.values[:, 0] - top.values[:, 1]], 1).to(torch.float32)


def clips_tempogram(args, api):
    """--tempogram: 64 clips of 30 s (--clips / --clip-frames change that) at 22 050 Hz mono as onset envelope [K, 1, 1292],
    tempogram [K, 1, 384, 1292] and tempo [K, 1, 4] with librosa's defaults (n_fft 2048, hop 512, 128 bands, lag 1, max_size 1,
    window 384, prior 120 bpm) in device memory, run after run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the spans of the
    widened clips; (b) pdmp3_amd_bulk_decode_clips_mel_long for the widened clips; (c) per mode, (b) -- for mode 0 on the clips
    widened by the lag alone -- followed by the same algorithm in torch on the device: diff, relu, mean, unfold, window,
    torch.fft autocorrelation, normalise, mean, log1p, prior, topk; (d) per mode, pdmp3_amd_bulk_decode_clips_tempogram.  (c) and
    (d) are compared once (largest differences and the share of clips with the same lag, printed, not asserted: the tests check
    (d) against the definition).  The kernels' own times come from a kernel-trace run of this mode
    (profiles/clip_tempogram.txt).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, Fm, rate, N, H, nm, lag, wt = args.clips, args.clip_frames, 22050, 2048, 512, 128, 1, 384
    span = 30 * rate if Fm == 1149 else Fm * 1152 * rate // 44100
    F = span // H + 1
    front, back, tiles, ksteps, frames_wg, lds = api.tempogram_plan(rate)
    Fw = F + front + back                                                       # frames of the widened clips
    T = (Fw - 1) * H + N
    sel = clip_selection(args, ixs, first=400, margin=4)
    clips, wide, wide0, spans = [], [], [], []
    for i, a in sel:
        start = clip_start(ixs[i], a, rate)
        assert start - front * H - N // 2 >= 0
        clips.append((files[i], ixs[i], start))
        wide.append((files[i], ixs[i], start - front * H))
        wide0.append((files[i], ixs[i], start - lag * H))
        spans.append((files[i], ixs[i], start - front * H - N // 2))
    dev = "cuda:0"
    sig = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    mel = torch.zeros((K, 1, nm, Fw), dtype=torch.float32, device=dev)
    mel0 = torch.zeros((K, 1, nm, F + lag), dtype=torch.float32, device=dev)
    shapes = {"onset": (F,), "tempogram": (wt, F), "tempo": (4,)}
    out_t = {}
    out_p = {m: torch.zeros((K, 1) + sh, dtype=torch.float32, device=dev) for m, sh in shapes.items()}
    window = torch.from_numpy(api.tempogram_window(wt)).to(dev)
    prior = torch.from_numpy(api.tempogram_prior(rate)[0]).to(dev)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(spans, T, rate, 1, out=sig)

    def mel_route():
        dec.decode_clips_mel_long(wide, Fw, rate, N, H, nm, out=mel)

    def torch_route(mode):
        def run():
            if mode == "onset":
                dec.decode_clips_mel_long(wide0, F + lag, rate, N, H, nm, out=mel0)
                out_t[mode] = torch_tempogram(mel0[:, 0], lag, wt, F, window, prior, rate, H, 0)
            else:
                dec.decode_clips_mel_long(wide, Fw, rate, N, H, nm, out=mel)
                out_t[mode] = torch_tempogram(mel[:, 0], lag, wt, F, window, prior, rate, H, 1 if mode == "tempogram" else 2)
            torch.cuda.synchronize()
        return run

    def product_route(mode):
        return lambda: dec.decode_clips_tempogram(clips, F, rate, N, H, nm, lag, 1, wt, out_mode=mode, out=out_p[mode])

    routes = [("audio clips", audio_route), ("mel_long clips", mel_route)]
    for m in shapes:
        routes += [("mel_long clips + torch " + m, torch_route(m)), ("tempogram clips, " + m, product_route(m))]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(
        {"largest_onset_difference": float((out_t["onset"] - out_p["onset"][:, 0]).abs().max()),
         "largest_onset": float(out_p["onset"].max()),
         "largest_tempogram_difference": float((out_t["tempogram"] - out_p["tempogram"][:, 0]).abs().max()),
         "clips": K, "clips_with_torchs_lag": int((out_t["tempo"][:, 1] == out_p["tempo"][:, 0, 1]).sum()),
         "bpm": sorted(set(round(float(v), 2) for v in out_p["tempo"][:, 0, 0].cpu()))[:8]}))
    dec.close()
    res = {"workload": "%d clips of %d frames at %d Hz mono, n_fft %d hop %d, %d bands, lag %d, tempogram window %d (%d log-mel frames a clip): %s" % (
               K, F, rate, N, H, nm, lag, wt, Fw, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "plan": {"frames_in_front": front, "frames_behind": back, "lag_tiles": tiles, "matrix_instructions_a_tile": ksteps,
                    "frames_a_workgroup": frames_wg, "lds_bytes": lds},
           "matrix_instructions": K * F * tiles * ksteps, "stage_bytes": {"log_mel": K * nm * Fw * 4, "envelope": K * (F + wt - 1) * 4, "tempogram": K * wt * F * 4},
           "seen": seen, "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    for m in shapes:
        res[m + "_minus_mel_long_ms"] = round((med["tempogram clips, " + m] - med["mel_long clips"]) * 1e3, 3)
        res[m + "_torch_minus_mel_long_ms"] = round((med["mel_long clips + torch " + m] - med["mel_long clips"]) * 1e3, 3)
    res["largest_spread_ms"] = round(max(max(ts) - min(ts) for ts in times.values()) * 1e3, 3)
    close()
    print(json.dumps(res))


def clips_fbank(args, api):
    """--clips K --clip-frames F --fbank: the clips of clips() (same seed, same places), the whole seconds of F MPEG-1 frames'
    length each, as Kaldi-style filterbank features [K, 1, frames, 80] at 16 kHz mono (25 ms povey frames every 10 ms, N = 512,
    ln) in device memory, three ways, run after run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the same spans (the call
    the feature call makes itself); (b) (a) followed by the chain of torch kernels that computes the same definition for the
    whole batch -- unfold, mean, pre-emphasis, window, pad, rfft, abs() ** 2, matmul, log; a dense matmul against the plain
    DFT where torch.fft cannot run --; (c) pdmp3_amd_bulk_decode_clips_fbank.  (b) and (c) are compared once (largest
    difference of the ln values above -10, printed, not asserted: the tests check (c) against the definition).  Medians and
    min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, nw, hop, n_mels, rho = args.clips, args.clip_frames, 16000, 400, 160, 80, 0.97
    n = api.fbank_dft_length(nw)
    sel = clip_selection(args, ixs)
    seconds = max(F * 1152 // 44100, 1)
    Fm = 1 + (seconds * rate - nw) // hop                                          # (Kaldi's snip_edges count: 2998 for 30 s)
    T = (Fm - 1) * hop + nw
    dev = "cuda:0"
    clips = [(files[i], ixs[i], clip_start(ixs[i], a, rate)) for i, a in sel]
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_t = torch.zeros((K, 1, Fm, n_mels), dtype=torch.float32, device=dev)
    out_f = torch.zeros((K, 1, Fm, n_mels), dtype=torch.float32, device=dev)
    t = 2.0 * np.pi * np.arange(nw) / (nw - 1)
    window = torch.from_numpy(((0.5 - 0.5 * np.cos(t)) ** 0.85).astype(np.float32)).to(dev)
    fbt = torch.from_numpy(api.fbank_filterbank(rate, n, n_mels).T.copy()).to(dev)                     # [N / 2, n_mels]
    ang = 2.0 * np.pi * ((np.arange(nw)[:, None] * np.arange(n // 2)[None, :]) % n) / n
    plain = torch.from_numpy(np.hstack([np.cos(ang), -np.sin(ang)]).astype(np.float32)).to(dev)        # [Nw, N]: Re | Im
    eps = float(np.finfo(np.float32).eps)
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()
    how = {"dft": "torch.fft.rfft"}

    def audio_route():
        dec.decode_clips_audio(clips, T, rate, 1, out=out_a)

    def torch_route():
        dec.decode_clips_audio(clips, T, rate, 1, out=out_a)
        fr = out_a[:, 0].unfold(1, nw, hop)                                                               # [K, Fm, Nw]
        fr = fr - fr.mean(dim=2, keepdim=True)
        fr = fr - rho * torch.nn.functional.pad(fr, (1, 0), mode="replicate")[:, :, :-1]
        fr = fr * window
        if how["dft"] == "torch.fft.rfft":
            try:
                p = torch.fft.rfft(torch.nn.functional.pad(fr, (0, n - nw)), dim=2).abs()[:, :, :n // 2] ** 2
            except Exception as e:                      # noqa: BLE001  (no FFT library on this build)
                how["dft"] = "dense matmul against the plain DFT (torch.fft.rfft: %s)" % type(e).__name__
        if how["dft"] != "torch.fft.rfft":
            x = fr @ plain
            p = x[:, :, :n // 2] ** 2 + x[:, :, n // 2:] ** 2
        out_t[:, 0] = torch.log(torch.clamp(p @ fbt, min=eps))
        torch.cuda.synchronize()

    def fbank_route():
        dec.decode_clips_fbank(clips, Fm, rate, win_length=nw, hop=hop, num_mel_bins=n_mels, out=out_f)

    routes = [("audio clips", audio_route), ("audio clips + torch chain", torch_route), ("fbank clips", fbank_route)]
    seen = {}

    def compare():
        big = out_t > -10.0
        seen["diff"] = float((out_t - out_f)[big].abs().max()) if bool(big.any()) else 0.0
    times = time_routes(routes, args.warmup_runs, args.runs, compare)
    dec.close()
    res = {"workload": "%d clips of %d frames' length as %d frames x %d bins at %d Hz mono (Nw %d, hop %d, N %d, povey, ln): %s" % (
               K, F, Fm, n_mels, rate, nw, hop, n, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs, "torch_chain": how["dft"],
           "largest_difference_of_the_two_ln_results_above_minus_10": seen["diff"], "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    b = times["audio clips + torch chain"]
    res["fbank_minus_audio_ms"] = round((statistics.median(times["fbank clips"]) - statistics.median(times["audio clips"])) * 1e3, 3)
    res["torch_chain_minus_audio_ms"] = round((statistics.median(b) - statistics.median(times["audio clips"])) * 1e3, 3)
    res["fbank_faster_than_torch_chain_by_more_than_its_spread"] = bool(statistics.median(b) - statistics.median(times["fbank clips"]) > max(b) - min(b))
    close()
    print(json.dumps(res))


def clips_mfcc(args, api):
    """--clips K --clip-frames F --mfcc: the clips of clips_fbank() (same seed, same places, same frames) as Kaldi-style MFCC
    features [K, 1, frames, 13] at 16 kHz mono (25 ms povey frames every 10 ms, N = 512, 23 bands, lifter 22) in device memory,
    three ways, run after run in turn: (a) pdmp3_amd_bulk_decode_clips_audio for the same spans (the call the feature calls
    make themselves); (b) pdmp3_amd_bulk_decode_clips_fbank for the 23 log bands followed by torch.matmul with the DCT table
    the loader builds itself (lifter folded in, as pdmp3_amd_mfcc_dct_table gives it) and the copy into the output -- what a
    loader does today; (c) pdmp3_amd_bulk_decode_clips_mfcc.  (b) and (c) are compared once (largest difference, printed, not
    asserted: the tests check (c) against the definition).  Medians and min..max of --runs runs."""
    import torch
    files, ixs, close = clip_corpus(args, api)
    K, F, rate, nw, hop, n_mels, n_ceps, lift = args.clips, args.clip_frames, 16000, 400, 160, 23, 13, 22.0
    sel = clip_selection(args, ixs)
    seconds = max(F * 1152 // 44100, 1)
    Fm = 1 + (seconds * rate - nw) // hop
    T = (Fm - 1) * hop + nw
    dev = "cuda:0"
    clips = [(files[i], ixs[i], clip_start(ixs[i], a, rate)) for i, a in sel]
    out_a = torch.zeros((K, 1, T), dtype=torch.float32, device=dev)
    out_l = torch.zeros((K, 1, Fm, n_mels), dtype=torch.float32, device=dev)
    out_t = torch.zeros((K, 1, Fm, n_ceps), dtype=torch.float32, device=dev)
    out_c = torch.zeros((K, 1, Fm, n_ceps), dtype=torch.float32, device=dev)
    dct = torch.from_numpy(api.mfcc_dct_table(n_mels, n_ceps, lift)[:n_mels, :n_ceps].copy()).to(dev)      # [n_mels, n_ceps]
    dec = api.BulkDecoder(threads=args.clip_threads)
    torch.cuda.synchronize()

    def audio_route():
        dec.decode_clips_audio(clips, T, rate, 1, out=out_a)

    def fbank_route():
        dec.decode_clips_fbank(clips, Fm, rate, win_length=nw, hop=hop, num_mel_bins=n_mels, out=out_l)
        torch.matmul(out_l, dct, out=out_t)
        torch.cuda.synchronize()

    def mfcc_route():
        dec.decode_clips_mfcc(clips, Fm, rate, n_ceps, lift, n_mels, win_length=nw, hop=hop, out=out_c)

    routes = [("audio clips", audio_route), ("fbank clips + torch.matmul", fbank_route), ("mfcc clips", mfcc_route)]
    seen = {}
    times = time_routes(routes, args.warmup_runs, args.runs, lambda: seen.update(diff=float((out_t - out_c).abs().max())))
    dec.close()
    res = {"workload": "%d clips of %d frames' length as %d frames x %d cepstra of %d bands at %d Hz mono (Nw %d, hop %d, povey, lifter %g): %s" % (
               K, F, Fm, n_ceps, n_mels, rate, nw, hop, lift, corpus_name(args, files)),
           "source_rates": sorted(set(ixs[i].rate for i, _ in sel)), "destination": "device memory", "runs": args.runs,
           "largest_difference_of_the_two_results": seen["diff"], "host_cpus": os.cpu_count()}
    res.update(route_stats(times, K))
    b = times["fbank clips + torch.matmul"]
    res["mfcc_minus_audio_ms"] = round((statistics.median(times["mfcc clips"]) - statistics.median(times["audio clips"])) * 1e3, 3)
    res["fbank_matmul_minus_audio_ms"] = round((statistics.median(b) - statistics.median(times["audio clips"])) * 1e3, 3)
    res["mfcc_faster_than_fbank_matmul_by_more_than_its_spread"] = bool(statistics.median(b) - statistics.median(times["mfcc clips"]) > max(b) - min(b))
    close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--threads", default="1,4,8")
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--parse-only", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--c4", type=int, default=0, metavar="JOBS",
                    help="SURVEY 8d C4 instead: the mixed corpus (64 files x >= 4096 frames), JOBS decoders in parallel")
    ap.add_argument("--device-out", action="store_true", help="PCM into device memory (torch tensors): it never leaves the GPU")
    ap.add_argument("--pinned", action="store_true", help="PCM into pinned host buffers (pdmp3_amd_pcm_alloc): no host copy")
    ap.add_argument("--gpus", type=int, default=1, help="--c4: decoder j runs on GPU j %% GPUS")
    ap.add_argument("--host-huffman", action="store_true", help="scalefactors + Huffman on the host pool instead of the device")
    ap.add_argument("--lsf", type=int, default=0, choices=(0, 1, 2), metavar="VERSION",
                    help="an MPEG-2 LSF (1) or MPEG-2.5 (2) stream at --sfreq, joint stereo 64 kbps, decoded with PDMP3_ISO_LSF")
    ap.add_argument("--sfreq", type=int, default=0, choices=(0, 1, 2), help="--lsf: the header's sampling-frequency field")
    ap.add_argument("--clips", type=int, default=0, metavar="K",
                    help="K clips (pdmp3_amd_bulk_decode_clips) at random places in the C4 corpus into device memory, against "
                         "decoding the whole files and slicing (see clips())")
    ap.add_argument("--clip-frames", type=int, default=191, metavar="F", help="--clips: frames per clip (191: 5 s at 44.1 kHz)")
    ap.add_argument("--c3", action="store_true", help="--clips: out of the C3 file (one hour) instead of the C4 corpus")
    ap.add_argument("--runs", type=int, default=12, help="--clips: timed runs of each route (medians, min, max)")
    ap.add_argument("--warmup-runs", type=int, default=2)
    ap.add_argument("--clip-threads", type=int, default=0, help="--clips: the decoders' copy threads (0: the library's choice)")
    ap.add_argument("--seed", type=int, default=20261016)
    ap.add_argument("--audio", type=int, default=0, metavar="RATE",
                    help="--clips: the clips as one float32 batch at RATE (pdmp3_amd_bulk_decode_clips_audio) against the plain clip "
                         "call and against the plain call followed by torch kernels (see clips_audio())")
    ap.add_argument("--mono", action="store_true", help="--audio: downmixed to one channel")
    ap.add_argument("--mel", action="store_true",
                    help="--clips: the clips as log-mel features at 16 kHz mono (pdmp3_amd_bulk_decode_clips_mel) against the audio call "
                         "for the same samples and against that call followed by torch kernels (see clips_mel())")
    ap.add_argument("--stft", action="store_true",
                    help="--clips: the clips' short-time Fourier transform at 16 kHz mono (pdmp3_amd_bulk_decode_clips_stft) against the audio "
                         "call alone and the audio call followed by torch.stft")
    ap.add_argument("--stft-long", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as their short-time Fourier transform at 44.1 kHz mono, n_fft 2048, "
                         "hop 512 (pdmp3_amd_bulk_decode_clips_stft_long) against the audio call alone and the audio call followed by torch.stft")
    ap.add_argument("--mel-long", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as 128 x 2583 log10-mel frames at 44.1 kHz mono, n_fft 2048, hop 512 "
                         "(pdmp3_amd_bulk_decode_clips_mel_long) against the audio call alone, the audio call followed by torch kernels, and "
                         "pdmp3_amd_bulk_decode_clips_stft_long's powers followed by a matmul and log10 (see clips_mel_long())")
    ap.add_argument("--cqt", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as 84 x 1292 constant-Q magnitudes at 22 050 Hz mono, C1, 12 bins an "
                         "octave, hop 512 (pdmp3_amd_bulk_decode_clips_cqt) against the audio call alone and the audio call followed by a "
                         "dense torch matmul over unfolded frames (see clips_cqt())")
    ap.add_argument("--chroma", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as 12 x 1292 chroma features at 22 050 Hz mono, the default spec "
                         "(pdmp3_amd_bulk_decode_clips_chroma) against the audio call alone and the constant-Q call followed by the fold and "
                         "the max norm in torch (see clips_chroma())")
    ap.add_argument("--loudness", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) at 32 000 Hz stereo measured by ITU-R BS.1770 and scaled to -14 LUFS "
                         "(pdmp3_amd_bulk_decode_clips_loudness) against the audio call alone (see clips_loudness())")
    ap.add_argument("--r128", action="store_true",
                    help="--loudness's batch with pdmp3_amd_bulk_decode_clips_r128 (true peak, short-term loudness, loudness range, the gain "
                         "held to -1 dBTP) as a third route beside the loudness call and the audio call (see clips_loudness())")
    ap.add_argument("--pitch", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as YIN pitch [3, 1292] at 22 050 Hz mono with librosa.yin's defaults "
                         "(pdmp3_amd_bulk_decode_clips_pitch) against the audio call alone and the audio call followed by the same algorithm "
                         "in torch on the device (see clips_pitch())")
    ap.add_argument("--pyin", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) through pYIN at 22 050 Hz mono with librosa.pyin's defaults "
                         "(pdmp3_amd_bulk_decode_clips_pyin, both modes) against the audio call alone and against the pitch call's curve "
                         "(see clips_pyin())")
    ap.add_argument("--beat", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) through the beat tracker at 22 050 Hz mono with librosa's defaults "
                         "(pdmp3_amd_bulk_decode_clips_beats, tempo estimated and given) against the tempogram call's onset and tempo modes and "
                         "against the onset mode followed by a copy to the host and the numpy restatement (see clips_beat())")
    ap.add_argument("--tempogram", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as onset envelope, tempogram [384, 1292] and tempo at 22 050 Hz mono with "
                         "librosa's defaults (pdmp3_amd_bulk_decode_clips_tempogram, all three modes) against the audio call alone, the log-mel "
                         "call alone and that call followed by the same algorithm in torch on the device (see clips_tempogram())")
    ap.add_argument("--spectral", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as 6 x 2583 spectral descriptors at 44.1 kHz mono, n_fft 2048, hop 512 "
                         "(pdmp3_amd_bulk_decode_clips_spectral) against the audio call alone, the audio call followed by torch kernels, and "
                         "pdmp3_amd_bulk_decode_clips_stft_long's magnitudes followed by the reductions in torch (see clips_spectral())")
    ap.add_argument("--hpss", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as harmonic and percussive soft masks [2, 1025, 1292] at 22 050 Hz mono, "
                         "n_fft 2048, hop 512, kernels 31 / 31, power 2 (pdmp3_amd_bulk_decode_clips_hpss) against the audio call alone, "
                         "pdmp3_amd_bulk_decode_clips_stft_long's magnitudes alone and those followed by the same algorithm in torch (see clips_hpss())")
    ap.add_argument("--mfcc-long", action="store_true",
                    help="64 clips of 30 s (or --clips / --clip-frames) as librosa's MFCC with delta and delta-delta [60, 1292] at 22 050 Hz mono, "
                         "n_fft 2048, hop 512, 128 bands, top_db 80 (pdmp3_amd_bulk_decode_clips_mfcc_long) against "
                         "pdmp3_amd_bulk_decode_clips_mel_long alone and that call followed by the same chain in torch (see clips_mfcc_long())")
    ap.add_argument("--fbank", action="store_true",
                    help="--clips: the clips as Kaldi-style filterbank features at 16 kHz mono (pdmp3_amd_bulk_decode_clips_fbank) against "
                         "the audio call for the same spans and against that call followed by torch kernels (see clips_fbank())")
    ap.add_argument("--mfcc", action="store_true",
                    help="--clips: the clips as Kaldi-style MFCC features at 16 kHz mono (pdmp3_amd_bulk_decode_clips_mfcc) against the "
                         "audio call for the same spans and against the fbank call followed by torch.matmul (see clips_mfcc())")
    args = ap.parse_args()
    if args.stft_long or args.mel_long or args.cqt or args.chroma or args.loudness or args.r128 or args.pitch or args.pyin or args.beat or args.tempogram or args.spectral or args.hpss or args.mfcc_long:
        args.clips = args.clips or 64
        if not any(a.startswith("--clip-frames") for a in sys.argv[1:]):
            args.clip_frames = 1149
    if args.clips:
        from pdmp3_amd import api
        if args.cqt:
            return clips_cqt(args, api)
        if args.chroma:
            return clips_chroma(args, api)
        if args.loudness or args.r128:
            return clips_loudness(args, api, r128=args.r128)
        if args.pitch:
            return clips_pitch(args, api)
        if args.pyin:
            return clips_pyin(args, api)
        if args.beat:
            return clips_beat(args, api)
        if args.tempogram:
            return clips_tempogram(args, api)
        if args.mel_long:
            return clips_mel_long(args, api)
        if args.spectral:
            return clips_spectral(args, api)
        if args.hpss:
            return clips_hpss(args, api)
        if args.mfcc_long:
            return clips_mfcc_long(args, api)
        if args.stft or args.stft_long:
            return clips_stft(args, api, long=args.stft_long)
        if args.mfcc:
            return clips_mfcc(args, api)
        if args.fbank:
            return clips_fbank(args, api)
        return clips_mel(args, api) if args.mel else clips_audio(args, api) if args.audio else clips(args, api)
    if args.lsf and (args.parse_only or args.c4):
        ap.error("--lsf: whole-stream decodes of one stream only")
    from pdmp3_amd.packer import packer
    from pdmp3_amd import api
    if args.c4:
        return c4(args, api)
    t0 = time.perf_counter()
    if args.lsf:
        mp3 = packer.generate(n_frames=args.frames, seed=0xC3, version=args.lsf, sfreq=args.sfreq, mode=1, mode_ext=2, bitrate_index=8)
    else:
        mp3 = packer.generate(n_frames=args.frames, seed=0xC3, sfreq=0, mode=1, mode_ext=2, bitrate_index=14)
    iso = api.ISO_LSF if args.lsf else 0
    a = np.frombuffer(mp3, dtype=np.uint8)
    t_gen = time.perf_counter() - t0
    t0 = time.perf_counter()
    total, frames = api.scan_buffer(a, iso)
    t_scan = time.perf_counter() - t0
    rate = [[44100, 48000, 32000], [22050, 24000, 16000], [11025, 12000, 8000]][args.lsf][args.sfreq if args.lsf else 0]
    rt = rate / (576.0 if args.lsf else 1152.0)
    out = {"frames": frames, "mp3_bytes": len(mp3), "pcm_bytes": total, "packer_s": round(t_gen, 2), "rate": rate,
           "stream": ("MPEG-2 LSF" if args.lsf == 1 else "MPEG-2.5") + " joint stereo 64 kbps" if args.lsf else "MPEG-1 joint stereo 320 kbps",
           "scan_ms": round(t_scan * 1e3, 2), "scan_frames_per_s": round(frames / t_scan, 1), "host_cpus": os.cpu_count(),
           "runs": []}
    pin = api.PinnedPCM(total // 2) if args.pinned else None
    pcm = pin.array if pin else np.empty(total // 2, dtype=np.int16)
    dout = None
    if args.device_out:                        # PCM stays in HBM (a torch tensor as the destination)
        import torch
        dout = torch.empty(max(total, 2) // 2, dtype=torch.int16, device="cuda:0")
    for th in [int(x) for x in args.threads.split(",")]:
        b = api.BulkDecoder(threads=th, window_frames=args.window, parse_only=args.parse_only, host_huffman=args.host_huffman)
        if iso:
            b.set_quirks(iso)
        best = None
        for _ in range(args.reps):
            t0 = time.perf_counter()
            if args.parse_only:
                b.parse(a)
            elif dout is not None:
                got, _, _ = b.decode_into_device(a, dout, wait=True)
                assert got == total
            else:
                got, _, _ = b.decode_into(a, pcm)
                assert got == total
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        huff = b.huffman_frames() if not args.parse_only else (0, 0)
        b.close()
        out["runs"].append({"threads": th, "seconds": round(best, 4), "frames_per_s": round(frames / best, 1),
                            "huffman_frames_device_host": list(huff),
                            "x_realtime": round(frames / best / rt, 1), "mode": "parse" if args.parse_only else ("decode, host Huffman" if args.host_huffman else "decode, device Huffman"),
                            "pcm": "device" if dout is not None else "pinned" if args.pinned else "pageable"})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
