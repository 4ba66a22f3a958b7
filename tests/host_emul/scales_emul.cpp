// scales_emul.cpp -- CPU build of the granule kernel's band-scale tables (pdmp3_amd/csrc/decode_core.h ScaleTabs,
// ph_scales_tab; host_tables.h builds them) for the test-suite.
//
// TEST INFRASTRUCTURE (tests/test_scales_tables_host.py, tests/test_gran_scales_emul.py).  emul.cpp's granule launch hands
// run_granule_wave no ScaleTabs, so the band scales are computed there; the launch here is its twin WITH the tables, loaded
// the way engine.hip's gran_workgroup loads them.  Never loaded by the product (pdmp3_amd/).
#include "wave_emul.h"
#include "../../pdmp3_amd/csrc/decode_core.h"
#include "../../pdmp3_amd/csrc/host_tables.h"

#include <memory>
#include <vector>

using namespace pdmp3;

static HostTables& host_tables() {
  static HostTables H;
  static bool ready = false;
  if (!ready) { build_host_tables(H); ready = true; }
  return H;
}
static const ScaleTabs& scale_tabs() { return *reinterpret_cast<const ScaleTabs*>(&host_tables().tab_image[kNumSfreq]); }

extern "C" int scales_emul_forms_exact() { return host_tables().ldexp_forms_exact ? 1 : 0; }

// t1 over n = 0 .. n_max, t2 over k = -266 .. 45, as ph_scales_tab indexes them: mismatches against the functions
extern "C" int scales_emul_check_tables(int n_max) {
  const ScaleTabs& G = scale_tabs();
  int bad = 0;
  for (int n = 0; n <= n_max; n++)
    if (f2u(G.t1[n < kScaleT1Max ? n : kScaleT1Max]) != f2u(pow2_neg_half((uint32_t)n))) bad++;
  for (int k = kScaleT2Min; k <= kScaleT2Max; k++)
    if (f2u(G.t2[k - kScaleT2Min]) != f2u(pow2_quarter(k))) bad++;
  return bad;
}
extern "C" void scales_emul_lane_consts(uint32_t* out) { for (int l = 0; l < 64; l++) out[l] = scale_tabs().lane[l]; }

// both forms of the band scales on one pair of side records and the peek values given: L.scale of either, as uint32
extern "C" void scales_emul_both(const uint8_t* side0, const uint8_t* side1, const float* peek, uint32_t* formula, uint32_t* table) {
  static WaveData L;
  memcpy(L.side[0], side0, 128);
  memcpy(L.side[1], side1, 128);
  for (int i = 0; i < 4; i++) L.peek[i] = peek[i];
  for (int pass = 0; pass < 2; pass++) {
    memset(L.scale, 0xa5, sizeof L.scale);
    for (int lane = 0; lane < 64; lane++) { if (pass) ph_scales_tab(lane, L, scale_tabs()); else ph_scales(lane, L); }
    memcpy(pass ? table : formula, L.scale, sizeof L.scale);
  }
}

// The exhaustive sweep, here and not in Python for its length.  Scalefactor bytes `vals` (n_vals of them) go round the
// records' scalefactor places -- place i of channel ch holds vals[(i + shift + 3 ch) % n_vals], every shift -- so that every
// place, the H5 mark included, sees every value beside different neighbours; flag bytes: scalefac_scale x preflag x
// long / short / mixed; subblock_gain (g, g + 1, g + 2) mod 8 for g = 0..7; the peek values `peeks`, rotated over the three
// windows; global_gain from `gains`.  -> number of (configuration, channel, band) whose two forms differ in a bit.
extern "C" long scales_emul_sweep(const uint8_t* vals, int n_vals, const float* peeks, int n_peeks, const uint8_t* gains, int n_gains,
                                  long* n_checked) {
  static WaveData L;
  const ScaleTabs& G = scale_tabs();
  static const unsigned kBlock[3] = {0u, PDMP3_GC_WIN_SWITCH | (2u << PDMP3_GC_BLOCK_TYPE_SHIFT), PDMP3_GC_WIN_SWITCH | (2u << PDMP3_GC_BLOCK_TYPE_SHIFT) | PDMP3_GC_MIXED};
  long bad = 0, checked = 0;
  uint32_t a[2][64], b[2][64];
  for (int gi = 0; gi < n_gains; gi++)
    for (int fl = 0; fl < 4; fl++)
      for (int bk = 0; bk < 3; bk++)
        for (int sbg = 0; sbg < 8; sbg++)
          for (int shift = 0; shift < n_vals; shift++)
            for (int pk = 0; pk < n_peeks; pk++) {
              memset(L.side, 0, sizeof L.side);
              for (int ch = 0; ch < 2; ch++) {
                uint8_t* s = L.side[ch];
                s[2] = ch ? (uint8_t)(255 - gains[gi]) : gains[gi];
                s[3] = (uint8_t)((fl & 1 ? PDMP3_GC_SCALEFAC_SCALE : 0u) | (fl & 2 ? PDMP3_GC_PREFLAG : 0u) | kBlock[(bk + ch) % 3]);
                for (int w = 0; w < 3; w++) s[4 + w] = (uint8_t)((sbg + w + ch) & 7);
                for (int i = 8; i < 30 + 39; i++) s[i] = vals[(i + shift + 3 * ch) % n_vals];
              }
              for (int i = 0; i < 3; i++) L.peek[i] = peeks[(pk + i) % n_peeks];
              L.peek[3] = 0.0f;
              memset(L.scale, 0xa5, sizeof L.scale);
              for (int lane = 0; lane < 64; lane++) ph_scales(lane, L);
              memcpy(a, L.scale, sizeof a);
              memset(L.scale, 0xa5, sizeof L.scale);
              for (int lane = 0; lane < 64; lane++) ph_scales_tab(lane, L, G);
              memcpy(b, L.scale, sizeof b);
              for (int ch = 0; ch < 2; ch++)
                for (int e = 0; e < 64; e++) { checked++; if (a[ch][e] != b[ch][e]) bad++; }
            }
  *n_checked = checked;
  return bad;
}

// emul.cpp's emul_decode_frames_granules with the workgroup's ScaleTabs: one granule per wave, workgroups of 16
extern "C" int scales_emul_decode_frames_granules(const int16_t* spectra, const pdmp3_gc_side* side, int n_frames,
                                                  float* state, int16_t* pcm, float* pcm_f32, unsigned debug_flags, int sf_hint) {
  HostTables& H = host_tables();
  GlobalTables T{H.pow43.data(), H.linetab.data(), H.win.data(), H.frag_long.data(), H.frag_short.data(), H.frag_mat.data(), H.taps.data(), H.tab_image.data()};
  std::vector<float> state_next(kStateFloats);
  std::vector<float> cstate((size_t)n_frames * 2 * kGranFloats);
  std::vector<unsigned> cflag((size_t)n_frames * 4, 0u);
  DecodeArgs a{spectra, side, pcm, pcm_f32, state, state ? state_next.data() : nullptr, nullptr, n_frames, 1, nullptr,
               cstate.data(), cflag.data(), 7u, debug_flags, sf_hint};
  constexpr int WPW = 16;
  auto L = std::make_unique<WaveData[]>(WPW);
  auto S = std::make_unique<TabLds>();
  auto G = std::make_unique<ScaleTabs>();
  memset(G.get(), 0xa5, sizeof(ScaleTabs));
  emu::run_wave([&] { tab_load_image(emu::lane(), 64, *S, T, sf_hint); scale_tabs_load(emu::lane(), 64, *G, T); });
  unsigned tabs_ready = WPW;
  GranMb mb[WPW];
  for (int g0 = 0; g0 < 2 * n_frames; g0 += WPW) {
    const int nw = 2 * n_frames - g0 < WPW ? 2 * n_frames - g0 : WPW;
    memset(mb, 0, sizeof mb);
    std::function<void()> bodies[WPW];
    for (int w = 0; w < nw; ++w) {
      bodies[w] = [&, w] {
        const int g = g0 + w;
        const GranPos gp{L.get(), mb, w, WPW, &tabs_ready, 0, 0, 0, G.get()};
        LaneRegs pf;
        ph_prefetch(emu::lane(), pf, a.spectra + (size_t)g * 1152, a.side + (size_t)g * 2);
        if (pcm_f32) run_granule_wave<true, false, true>(a, T, &H.cb, g, L[w], *S, gp, pf);
        else run_granule_wave<false, false, true>(a, T, &H.cb, g, L[w], *S, gp, pf);
      };
    }
    emu::run_waves(bodies, nw);
  }
  if (state) std::copy(state_next.begin(), state_next.end(), state);
  return 0;
}
