// Host build of the true-peak instantiations of the loudness kernels (pdmp3_amd/csrc/loudness.hip k_loud_blocks<true>,
// k_loud_gate<true>) for tests/test_clip_r128_host.py, on top of loudness_emul.cpp: k_loud_states, k_loud_chain, the matrix
// instruction and the reduction tree are that file's (it is compiled into this one, so emul_clip_loudness is here too for the
// bit-for-bit comparison); the two kernels below follow the device's thread by thread with the pointwise arithmetic of
// loudness_core.h and r128_core.h.  LDS is a plain array poisoned at a workgroup's start: a float read that nobody had written,
// or a row of another wave, ends the run with -1.
#include "loudness_emul.cpp"

#include "../../pdmp3_amd/csrc/r128_core.h"

struct EmulR {
  Emul E;
  const float* taps;
  int n_st, n_rng, limit_tp;
};

static int blocks_group_tp(EmulR& R, int clip, int ch, int chunk) {
  Emul& E = R.E;
  const pdmp3_loud_params& P = E.P;
  std::vector<float> lds(PDMP3_LOUD_LDS_BYTES / sizeof(float), kPoison);
  const size_t row_i = (size_t)clip * P.channels + ch;
  const float* const row = row_of(E.descs[clip], ch);
  const float* const Hm = &E.tab->Hm[0][0];
  for (int wave = 0; wave < 4; wave++) {
    const long long tw = (long long)chunk * kLoudSpan + (long long)wave * kLoudWave;
    float peak[64], u[64][16], hi[64], lo[64], h[64][16], p[64][3], tp[64], v[64][3];
    for (int lane = 0; lane < 64; lane++) {
      peak[lane] = 0.0f;
      for (int it = 0; it < kLoudWave / 256; it++) {
        const int idx = it * 256 + 4 * lane;
        float x[4];
        load4(row, P.n_in, tw + idx, x);
        for (int e = 0; e < 4; e++) {
          peak[lane] = fmaxf(peak[lane], fabsf(x[e]));
          lds[loud_at(16 * wave + (idx >> 6), idx & 63) + e] = x[e];
        }
      }
    }
    for (int lane = 0; lane < 64; lane++) {
      const int j = lane & 15, kq = lane >> 4, bl = 16 * wave + j;
      for (int ks = 0; ks < 16; ks++) {
        u[lane][ks] = lds[loud_at(bl, 4 * ks + kq)];
        if (u[lane][ks] == kPoison) return -1;
      }
      const double* const sc = &E.starts[(row_i * P.n_chunks + chunk) * 4];
      const double from_rest = bl ? E.states[((row_i * P.n_chunks + chunk) * kLoudChunk + bl - 1) * 4 + kq] : 0.0;
      loud_split(loud_row_acc(E.tab->pow[bl], kq, sc, from_rest), &hi[lane], &lo[lane]);
      for (int n = 0; n < 16; n++) h[lane][n] = loud_hm(Hm, 4 * n - 12 + j - kq);
      p[lane][0] = p[lane][1] = p[lane][2] = 0.0f;
    }
    for (int mt = 0; mt < 4; mt++) {
      float acc[64][4], a[64], b[64];
      memset(acc, 0, sizeof acc);
      for (int ks = 0; ks < 4 * (mt + 1); ks++) {
        for (int lane = 0; lane < 64; lane++) { a[lane] = h[lane][4 * mt - ks + 3]; b[lane] = u[lane][ks]; }
        mfma(a, b, acc);
      }
      for (int lane = 0; lane < 64; lane++) { a[lane] = E.tab->O[16 * mt + (lane & 15)][lane >> 4]; b[lane] = hi[lane]; }
      mfma(a, b, acc);
      mfma(a, lo, acc);
      for (int lane = 0; lane < 64; lane++) {
        const int j = lane & 15, kq = lane >> 4;
        const long long tb = tw + (long long)j * kLoudB, ib = tb / P.q, edge = (ib + 1) * P.q;
        const int bin0 = (int)(ib - tw / P.q);
        if (bin0 < 0 || bin0 > 2) return -1;
        for (int r = 0; r < 4; r++) loud_square(acc[lane][r], tb + 16 * mt + 4 * kq + r, edge, bin0, p[lane]);
      }
    }
    // the interpolator
    for (int lane = 0; lane < 64; lane++) {
      const int j = lane & 15, kq = lane >> 4, bl = 16 * wave + j;
      tp[lane] = 0.0f;
      for (int n = 0; n < 3; n++) {
        if (j) {
          if (bl - 1 < 16 * wave) return -1;                     // (a row of another wave)
          v[lane][n] = lds[loud_at(bl - 1, 52 + 4 * n + kq)];
          if (v[lane][n] == kPoison) return -1;
        } else {
          v[lane][n] = r128_sample(row, P.n_in, tw - 12 + 4 * n + kq);
        }
      }
    }
    for (int ph = 1; ph <= 3; ph++) {
      float c[64][kR128Steps];
      for (int lane = 0; lane < 64; lane++)
        for (int n = 0; n < kR128Steps; n++) c[lane][n] = r128_tap(R.taps, ph, 4 * (n - 3) + (lane & 15) - (lane >> 4));
      for (int mt = 0; mt < 4; mt++) {
        float acc[64][4], a[64], b[64];
        memset(acc, 0, sizeof acc);
        for (int s = 0; s < kR128Steps; s++) {
          const int ks = 4 * mt - 3 + s;
          for (int lane = 0; lane < 64; lane++) { a[lane] = c[lane][6 - s]; b[lane] = ks < 0 ? v[lane][ks + 3] : u[lane][ks]; }
          mfma(a, b, acc);
        }
        for (int lane = 0; lane < 64; lane++) {
          const int j = lane & 15, kq = lane >> 4;
          const long long left = P.n_in - (tw + (long long)j * kLoudB);
          for (int r = 0; r < 4; r++)
            if (16 * mt + 4 * kq + r < left) tp[lane] = fmaxf(tp[lane], fabsf(acc[lane][r]));
        }
      }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      float np[64][3], npk[64], ntp[64];
      for (int lane = 0; lane < 64; lane++) {
        for (int n = 0; n < 3; n++) np[lane][n] = p[lane][n] + p[lane ^ off][n];
        npk[lane] = fmaxf(peak[lane], peak[lane ^ off]);
        ntp[lane] = fmaxf(tp[lane], tp[lane ^ off]);
      }
      memcpy(p, np, sizeof np);
      memcpy(peak, npk, sizeof npk);
      memcpy(tp, ntp, sizeof ntp);
    }
    float* const out = &E.part[((row_i * P.n_chunks + chunk) * 4 + wave) * kR128Part];
    out[0] = p[0][0]; out[1] = p[0][1]; out[2] = p[0][2]; out[3] = peak[0];
    out[4] = tp[0]; out[5] = out[6] = out[7] = 0.0f;
  }
  return 0;
}

static void gate_group_r128(EmulR& R, int clip, float* stats, float* mom, float* st) {
  Emul& E = R.E;
  const pdmp3_loud_params& P = E.P;
  const int C = P.channels, NT = kLoudGateThreads;
  const float* const part = &E.part[(size_t)clip * C * P.n_chunks * 4 * kR128Part];
  float* const sub = E.sub.data() + (size_t)clip * C * (size_t)P.n_sub;
  double a[NT], b[NT], c[NT];
  for (int tid = 0; tid < NT; tid++) {
    float pk = 0.0f, tpk = 0.0f;
    for (int ch = 0; ch < C; ch++) {
      const float* const pc = part + (size_t)ch * P.n_chunks * 4 * kR128Part;
      for (long long i = tid; i < P.n_sub; i += NT) sub[(size_t)ch * P.n_sub + i] = loud_sub_sum(pc, i, P.q, kR128Part);
      for (long long w = tid; w < (long long)P.n_chunks * 4; w += NT) {
        pk = fmaxf(pk, pc[w * kR128Part + 3]);
        tpk = fmaxf(tpk, pc[w * kR128Part + 4]);
      }
    }
    a[tid] = (double)pk;
    b[tid] = (double)tpk;
  }
  const double peak = reduce(a, true);
  const double tp = fmax(peak, reduce(b, true));
  for (int tid = 0; tid < NT; tid++) {
    a[tid] = b[tid] = 0.0; c[tid] = -INFINITY;
    for (long long j = tid; j < P.n_mom; j += NT) {
      const double z = loud_z(sub, P.n_sub, C, P.dual_mono, j, P.q), l = loud_l(z);
      if (mom) mom[j] = (float)l;
      c[tid] = fmax(c[tid], l);
      if (l > -70.0) { a[tid] += 1.0; b[tid] += z; }
    }
  }
  const double n_abs = reduce(a, false), sum_abs = reduce(b, false), top = reduce(c, true);
  const double gamma = n_abs > 0.0 ? loud_l(sum_abs / n_abs) - 10.0 : -INFINITY;
  for (int tid = 0; tid < NT; tid++) {
    a[tid] = b[tid] = 0.0;
    for (long long j = tid; j < P.n_mom; j += NT) {
      const double z = loud_z(sub, P.n_sub, C, P.dual_mono, j, P.q), l = loud_l(z);
      if (l > -70.0 && l > gamma) { a[tid] += 1.0; b[tid] += z; }
    }
  }
  const double n_rel = reduce(a, false), sum_rel = reduce(b, false);
  // the windows of 30, the range
  for (int tid = 0; tid < NT; tid++) {
    a[tid] = b[tid] = 0.0; c[tid] = -INFINITY;
    for (long long j = tid; j < R.n_st; j += NT) {
      const double w = loud_zn(sub, P.n_sub, C, P.dual_mono, j, P.q, kR128Window), S = loud_l(w);
      if (st) st[j] = (float)S;
      c[tid] = fmax(c[tid], S);
      if (j % kR128Every == 0 && S > -70.0) { a[tid] += 1.0; b[tid] += w; }
    }
  }
  const double s_top = reduce(c, true), n_ar = reduce(a, false), sum_ar = reduce(b, false);
  const double gamma_r = n_ar > 0.0 ? loud_l(sum_ar / n_ar) - 20.0 : -INFINITY;
  std::vector<double> vals(kR128MaxRange, (double)kPoison);
  for (int tid = 0; tid < NT; tid++) {
    a[tid] = 0.0;
    for (int m = tid; m < R.n_rng; m += NT) {
      const double S = loud_l(loud_zn(sub, P.n_sub, C, P.dual_mono, (long long)m * kR128Every, P.q, kR128Window));
      const bool in = S > -70.0 && S > gamma_r;
      vals[m] = in ? S : INFINITY;
      a[tid] += in ? 1.0 : 0.0;
    }
  }
  const double n_gr = reduce(a, false);
  double pick[2] = {0.0, 0.0};
  if (n_gr > 0.0) {
    const long long hi = r128_hi_index((long long)n_gr), lo = r128_lo_index((long long)n_gr);
    for (int m = 0; m < R.n_rng; m++) {
      if (vals[m] == INFINITY) continue;
      const long long r = r128_rank(vals.data(), R.n_rng, m);
      if (r == hi) pick[0] = vals[m];
      if (r == lo) pick[1] = vals[m];
    }
  }
  const double lra = n_gr > 0.0 ? pick[0] - pick[1] : 0.0;
  const double L = n_rel > 0.0 ? loud_l(sum_rel / n_rel) : -INFINITY;
  const float g = loud_gain(L, R.limit_tp ? tp : peak, P.target, P.peak_limit);
  stats[0] = (float)L; stats[1] = (float)top; stats[2] = (float)peak; stats[3] = g;
  stats[4] = (float)gamma; stats[5] = (float)P.n_mom; stats[6] = (float)n_abs; stats[7] = (float)n_rel;
  stats[8] = (float)tp; stats[9] = (float)s_top; stats[10] = (float)lra; stats[11] = (float)gamma_r;
  stats[12] = (float)R.n_st; stats[13] = (float)R.n_rng; stats[14] = (float)n_ar; stats[15] = (float)n_gr;
  E.gains[clip] = g;
}

extern "C" int emul_r128_params_bytes() { return (int)sizeof(pdmp3_r128_params); }
// the places of the two percentiles among n sorted values, as the kernels take them
extern "C" void emul_r128_indices(long long n, long long* hi, long long* lo) { *hi = r128_hi_index(n); *lo = r128_lo_index(n); }
// stats [n_clips][16]; mom NULL or [n_clips][n_mom]; st NULL or [n_clips][n_st]; 0, or -1 where the parameters are not the
// plan's or LDS is read unwritten
extern "C" int emul_clip_r128(const pdmp3_mel_desc* descs, int n_clips, const pdmp3_loud_tables* tab, const float* taps,
                              const pdmp3_r128_params* params, float* stats, float* mom, float* st) {
  const pdmp3_loud_params& P = params->loud;
  if (P.n_in <= 0 || P.n_in > 0x7fffffffLL || (P.channels != 1 && P.channels != 2) || P.q < 800 ||
      P.n_chunks != (P.n_in + kLoudSpan - 1) / kLoudSpan || P.n_sub != P.n_in / P.q || P.n_mom != (P.n_sub > 3 ? P.n_sub - 3 : 0))
    return -1;
  const int n_st = P.n_sub > kR128Window - 1 ? P.n_sub - (kR128Window - 1) : 0;
  if (params->n_st != n_st || params->n_rng != (n_st + kR128Every - 1) / kR128Every || params->n_rng > kR128MaxRange) return -1;
  EmulR R;
  Emul& E = R.E;
  R.taps = taps; R.n_st = params->n_st; R.n_rng = params->n_rng; R.limit_tp = params->limit_true_peak;
  E.descs = descs; E.tab = tab; E.P = P;
  const size_t rows = (size_t)n_clips * P.channels, chunks = rows * P.n_chunks;
  E.states.assign(chunks * kLoudChunk * 4, 0.0); E.starts.assign(chunks * 4, 0.0);
  E.part.assign(chunks * 4 * kR128Part, kPoison); E.sub.assign(rows * P.n_sub + 1, kPoison); E.gains.assign(n_clips, 0.0f);
  for (int k = 0; k < n_clips; k++)
    for (int ch = 0; ch < P.channels; ch++) {
      for (int c = 0; c < P.n_chunks; c++)
        if (states_wave(E, k, ch, c) != 0) return -1;
      chain_wave(E, k, ch);
      for (int c = 0; c < P.n_chunks; c++)
        if (blocks_group_tp(R, k, ch, c) != 0) return -1;
    }
  for (int k = 0; k < n_clips; k++) {
    gate_group_r128(R, k, stats + (size_t)k * 16, mom ? mom + (size_t)k * P.n_mom : nullptr, st ? st + (size_t)k * R.n_st : nullptr);
    for (int ch = 0; ch < P.channels; ch++) {
      const float* const row = row_of(descs[k], ch);
      float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(descs[k].dst)) + (size_t)ch * descs[k].dst_chan_stride;
      for (long long t = 0; t < P.n_in; t++) out[t] = row[t] * E.gains[k];
    }
  }
  return 0;
}
