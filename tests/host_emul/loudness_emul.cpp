// Host build of the loudness kernels (pdmp3_amd/csrc/loudness.hip) for tests/test_clip_loudness_host.py: the kernels' own
// indexing and pointwise arithmetic (pdmp3_amd/csrc/loudness_core.h) driven by the kernels' structure -- k_loud_states a wave a
// chunk with its lanes' shuffles as arrays over the 64 lanes, k_loud_chain a wave a row, k_loud_blocks four waves a chunk with
// each matrix instruction's result as the fused multiply-add chain it is (k ascending on top of C), the butterfly over the
// lanes, k_loud_gate's 256 threads and its reduction tree, k_loud_scale.  The addresses in the descriptors are host addresses
// here.  LDS is a plain array poisoned at a workgroup's start: a float read that nobody had written ends the run with -1.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../pdmp3_amd/csrc/loudness_core.h"

using namespace pdmp3;

static const float kPoison = -1e30f;

struct Emul {
  const pdmp3_mel_desc* descs;
  const pdmp3_loud_tables* tab;
  pdmp3_loud_params P;
  std::vector<double> states, starts;
  std::vector<float> part, sub, gains;
};

static const float* row_of(const pdmp3_mel_desc& d, int ch) {
  return reinterpret_cast<const float*>(static_cast<uintptr_t>(d.src)) + (size_t)ch * d.src_chan_stride;
}
static void load4(const float* row, long long T, long long t, float v[4]) {
  for (int e = 0; e < 4; e++) v[e] = loud_sample(row, T, t + e);
}

// loud_scan over the 64 lanes' states
static void scan(const pdmp3_loud_tables* tab, int level, double s[64][4]) {
  for (int k = 0; k < 6; k++) {
    const int d = 1 << k;
    double v[64][4];
    for (int l = 0; l < 64; l++) memcpy(v[l], s[l >= d ? l - d : l], sizeof v[l]);
    for (int l = d; l < 64; l++) loud_mat_acc(tab->pow[loud_pow_of(level, k)], v[l], s[l]);
  }
}

static int states_wave(Emul& E, int clip, int ch, int chunk) {
  const pdmp3_loud_params& P = E.P;
  std::vector<float> lds(kLoudChunk * kLoudRowS, kPoison);
  const size_t row_i = (size_t)clip * P.channels + ch;
  const float* const row = row_of(E.descs[clip], ch);
  const long long t0 = (long long)chunk * kLoudSpan;
  for (int lane = 0; lane < 64; lane++)
    for (int it = 0; it < kLoudSpan / 256; it++) {
      const int idx = it * 256 + 4 * lane;
      float v[4];
      load4(row, P.n_in, t0 + idx, v);
      for (int e = 0; e < 4; e++) lds[loud_at_s(idx >> 6, idx & 63) + e] = v[e];
    }
  double s[64][4];
  for (int lane = 0; lane < 64; lane++) {
    for (int j = 0; j < kLoudB; j++)
      if (lds[loud_at_s(lane, j)] == kPoison) return -1;
    loud_w(E.tab->R, lds.data() + loud_at_s(lane, 0), s[lane]);
  }
  scan(E.tab, 0, s);
  for (int lane = 0; lane < 64; lane++) memcpy(&E.states[((row_i * P.n_chunks + chunk) * kLoudChunk + lane) * 4], s[lane], sizeof s[lane]);
  memcpy(&E.starts[(row_i * P.n_chunks + chunk) * 4], s[63], sizeof s[63]);
  return 0;
}

static void chain_wave(Emul& E, int clip, int ch) {
  const pdmp3_loud_params& P = E.P;
  double* const e = &E.starts[((size_t)clip * P.channels + ch) * P.n_chunks * 4];
  double carry[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c0 = 0; c0 < P.n_chunks; c0 += 64) {
    double s[64][4];
    for (int lane = 0; lane < 64; lane++)
      for (int m = 0; m < 4; m++) s[lane][m] = c0 + lane < P.n_chunks ? e[(size_t)(c0 + lane) * 4 + m] : 0.0;
    loud_mat_acc(E.tab->pow[kLoudChunk], carry, s[0]);
    scan(E.tab, 1, s);
    for (int lane = 0; lane < 64; lane++)
      if (c0 + lane < P.n_chunks) memcpy(&e[(size_t)(c0 + lane) * 4], lane ? s[lane - 1] : carry, sizeof carry);
    memcpy(carry, s[63], sizeof carry);
  }
}

// v_mfma_f32_16x16x4_f32 over the wave: lane (j, kq) holds A[row j][k = kq], B[k = kq][col j], D[row 4 kq + r][col j]
static void mfma(const float a[64], const float b[64], float acc[64][4]) {
  for (int lane = 0; lane < 64; lane++) {
    const int j = lane & 15, kq = lane >> 4;
    for (int r = 0; r < 4; r++)
      for (int k = 0; k < 4; k++) acc[lane][r] = mel_fma(a[4 * kq + r + 16 * k], b[j + 16 * k], acc[lane][r]);
  }
}

static int blocks_group(Emul& E, int clip, int ch, int chunk) {
  const pdmp3_loud_params& P = E.P;
  std::vector<float> lds(PDMP3_LOUD_LDS_BYTES / sizeof(float), kPoison);
  const size_t row_i = (size_t)clip * P.channels + ch;
  const float* const row = row_of(E.descs[clip], ch);
  const float* const Hm = &E.tab->Hm[0][0];
  for (int wave = 0; wave < 4; wave++) {
    const long long tw = (long long)chunk * kLoudSpan + (long long)wave * kLoudWave;
    float peak[64], u[64][16], hi[64], lo[64], h[64][16], p[64][3];
    for (int lane = 0; lane < 64; lane++) {
      peak[lane] = 0.0f;
      for (int it = 0; it < kLoudWave / 256; it++) {
        const int idx = it * 256 + 4 * lane;
        float v[4];
        load4(row, P.n_in, tw + idx, v);
        for (int e = 0; e < 4; e++) {
          peak[lane] = fmaxf(peak[lane], fabsf(v[e]));
          lds[loud_at(16 * wave + (idx >> 6), idx & 63) + e] = v[e];
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
    for (int off = 32; off >= 1; off >>= 1) {
      float np[64][3], npk[64];
      for (int lane = 0; lane < 64; lane++) {
        for (int n = 0; n < 3; n++) np[lane][n] = p[lane][n] + p[lane ^ off][n];
        npk[lane] = fmaxf(peak[lane], peak[lane ^ off]);
      }
      memcpy(p, np, sizeof np);
      memcpy(peak, npk, sizeof npk);
    }
    float* const out = &E.part[((row_i * P.n_chunks + chunk) * 4 + wave) * 4];
    out[0] = p[0][0]; out[1] = p[0][1]; out[2] = p[0][2]; out[3] = peak[0];
  }
  return 0;
}

static double reduce(const double* v, bool is_max) {
  double red[kLoudGateThreads];
  memcpy(red, v, sizeof red);
  for (int n = kLoudGateThreads / 2; n >= 1; n >>= 1)
    for (int tid = 0; tid < n; tid++) red[tid] = is_max ? fmax(red[tid], red[tid + n]) : red[tid] + red[tid + n];
  return red[0];
}

static void gate_group(Emul& E, int clip, float* stats, float* mom) {
  const pdmp3_loud_params& P = E.P;
  const int C = P.channels, NT = kLoudGateThreads;
  const float* const part = &E.part[(size_t)clip * C * P.n_chunks * 16];
  float* const sub = E.sub.data() + (size_t)clip * C * (size_t)P.n_sub;
  double a[NT], b[NT], c[NT];
  for (int tid = 0; tid < NT; tid++) {
    float pk = 0.0f;
    for (int ch = 0; ch < C; ch++) {
      const float* const pc = part + (size_t)ch * P.n_chunks * 16;
      for (long long i = tid; i < P.n_sub; i += NT) sub[(size_t)ch * P.n_sub + i] = loud_sub_sum(pc, i, P.q);
      for (long long w = tid; w < (long long)P.n_chunks * 4; w += NT) pk = fmaxf(pk, pc[w * 4 + 3]);
    }
    a[tid] = (double)pk;
  }
  const double peak = reduce(a, true);
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
  const double L = n_rel > 0.0 ? loud_l(sum_rel / n_rel) : -INFINITY;
  const float g = loud_gain(L, peak, P.target, P.peak_limit);
  stats[0] = (float)L; stats[1] = (float)top; stats[2] = (float)peak; stats[3] = g;
  stats[4] = (float)gamma; stats[5] = (float)P.n_mom; stats[6] = (float)n_abs; stats[7] = (float)n_rel;
  E.gains[clip] = g;
}

extern "C" int emul_loudness_tables_bytes() { return (int)sizeof(pdmp3_loud_tables); }
extern "C" int emul_loudness_params_bytes() { return (int)sizeof(pdmp3_loud_params); }
// stats [n_clips][8]; mom NULL or [n_clips][n_mom]; 0, or -1 where the parameters are not the plan's or LDS is read unwritten
extern "C" int emul_clip_loudness(const pdmp3_mel_desc* descs, int n_clips, const pdmp3_loud_tables* tab, const pdmp3_loud_params* params,
                                  float* stats, float* mom) {
  const pdmp3_loud_params& P = *params;
  if (P.n_in <= 0 || P.n_in > 0x7fffffffLL || (P.channels != 1 && P.channels != 2) || P.q < 800 ||
      P.n_chunks != (P.n_in + kLoudSpan - 1) / kLoudSpan || P.n_sub != P.n_in / P.q || P.n_mom != (P.n_sub > 3 ? P.n_sub - 3 : 0))
    return -1;
  Emul E;
  E.descs = descs; E.tab = tab; E.P = P;
  const size_t rows = (size_t)n_clips * P.channels, chunks = rows * P.n_chunks;
  E.states.assign(chunks * kLoudChunk * 4, 0.0); E.starts.assign(chunks * 4, 0.0);
  E.part.assign(chunks * 16, kPoison); E.sub.assign(rows * P.n_sub + 1, kPoison); E.gains.assign(n_clips, 0.0f);
  for (int k = 0; k < n_clips; k++)
    for (int ch = 0; ch < P.channels; ch++) {
      for (int c = 0; c < P.n_chunks; c++)
        if (states_wave(E, k, ch, c) != 0) return -1;
      chain_wave(E, k, ch);
      for (int c = 0; c < P.n_chunks; c++)
        if (blocks_group(E, k, ch, c) != 0) return -1;
    }
  for (int k = 0; k < n_clips; k++) {
    gate_group(E, k, stats + (size_t)k * 8, mom ? mom + (size_t)k * P.n_mom : nullptr);
    for (int ch = 0; ch < P.channels; ch++) {
      const float* const row = row_of(descs[k], ch);
      float* const out = reinterpret_cast<float*>(static_cast<uintptr_t>(descs[k].dst)) + (size_t)ch * descs[k].dst_chan_stride;
      for (long long t = 0; t < P.n_in; t++) out[t] = row[t] * E.gains[k];
    }
  }
  return 0;
}
