// window_pairs_emul.cpp -- CPU build of the two forms of a stereo granule's window sums (pdmp3_amd/csrc/decode_core.h): the
// granule kernel's ph_window_own + ph_window_hist and the chunk kernels' ph_window_emit, on slots, history and taps given.
//
// TEST INFRASTRUCTURE (tests/test_window_pairs_emul.py).  Built twice: as it is (the granule form on register pairs) and
// with -DPD_EXP_WINDOW_SCALAR (eighteen scalar chains).  Never loaded by the product (pdmp3_amd/).
#include "wave_emul.h"
#include "../../pdmp3_amd/csrc/decode_core.h"
#include "../../pdmp3_amd/csrc/host_tables.h"

#include <memory>

using namespace pdmp3;

static HostTables& host_tables() {
  static HostTables H;
  static bool ready = false;
  if (!ready) { build_host_tables(H); ready = true; }
  return H;
}

extern "C" int window_pairs_emul_form() { return PD_GRAN_WINDOW_PAIRS; }

// slots [2 ch][18][33]: a granule's hyb as ph_overlap_matrix leaves it; he, ho [15][64 lanes]: the history of every lane.
//   pcm_gran, pcm_emit [1152]: the float PCM of either form -- the eighteen sums of every lane as they are, value
//     64 t + 2 i + ch the sum t of lane 32 ch + i;
//   hist_gran, hist_emit [2][15][64]: the history either form hands to the next granule (even-aged slots, then odd-aged):
//     the granule form's is read out of hyb HERE, at the places gran_send_rows and the closing state read (slots 3..17 at
//     idx_e / idx_o, before the sums are formed) -- the harness's own indexing, not the hand-over code: this says that
//     ph_window_emit's carried history is those slots.  A fault in
//     gran_send_rows or the closing-state code (both unchanged) would not show here; the state-block comparisons of
//     tests/test_gpu_gran_pairs.py and tests/test_gran_scales_emul.py run that code;
//   ref, ref_swapped [64][18]: the sums as plain chains of fmaf -- k ascending, we[k] before wo[k], and with wo[k] BEFORE
//     we[k] (a different order, for the test to see that the data can tell them apart)
extern "C" void window_pairs_emul(const float* slots, const float* he, const float* ho, float* pcm_gran, float* pcm_emit,
                                  float* hist_gran, float* hist_emit, float* ref, float* ref_swapped) {
  HostTables& H = host_tables();
  GlobalTables T{H.pow43.data(), H.linetab.data(), H.win.data(), H.frag_long.data(), H.frag_short.data(), H.frag_mat.data(), H.taps.data(), H.tab_image.data()};
  auto Lg = std::make_unique<WaveData>();
  auto Le = std::make_unique<WaveData>();
  auto S = std::make_unique<TabLds>();
  memcpy(Lg->hyb, slots, sizeof Lg->hyb);
  memcpy(Le->hyb, slots, sizeof Le->hyb);
  emu::run_wave([&] { tab_load_image(emu::lane(), 64, *S, T, 0); });
  emu::run_wave([&] {
    const int lane = emu::lane(), ch = lane >> 5;
    LaneRegs R;
    lane_init<false>(lane, *Lg, R, &H.cb, T);
    for (int s = 0; s < kHistSlots; s++) { R.he[s] = he[s * 64 + lane]; R.ho[s] = ho[s * 64 + lane]; }
    for (int s = 0; s < kHistSlots; s++) {
      hist_gran[s * 64 + lane] = Lg->hyb[ch][3 + s][R.idx_e];
      hist_gran[(kHistSlots + s) * 64 + lane] = Lg->hyb[ch][3 + s][R.idx_o];
    }
    PD_WAVE_SYNC();
#if PD_GRAN_WINDOW_PAIRS
    f32x2 tw[8], acc[9];
    ph_window_own(lane, *Lg, *S, R, tw, acc);
    ph_window_hist<true, true>(lane, *Lg, R, tw, acc, nullptr, pcm_gran);
#else
    float acc[18];
    ph_window_own(lane, *Lg, *S, R, acc);
    ph_window_hist<true, true>(lane, *Lg, R, acc, nullptr, pcm_gran);
#endif
  });
  emu::run_wave([&] {
    const int lane = emu::lane(), ch = lane >> 5;
    LaneRegs R;
    lane_init<true>(lane, *Le, R, &H.cb, T);
    for (int s = 0; s < kHistSlots; s++) { R.he[s] = he[s * 64 + lane]; R.ho[s] = ho[s * 64 + lane]; }
    // the plain chains: E[s], O[s], s = 0..14 the history, 15..32 the granule's slots
    float E[33], O[33];
    for (int s = 0; s < kHistSlots; s++) { E[s] = R.he[s]; O[s] = R.ho[s]; }
    for (int t = 0; t < 18; t++) { E[15 + t] = Le->hyb[ch][t][R.idx_e]; O[15 + t] = Le->hyb[ch][t][R.idx_o]; }
    for (int t = 0; t < 18; t++) {
      float a = 0.0f, b = 0.0f;
      for (int k = 0; k < 8; k++) {
        a = __builtin_fmaf(R.we[k], E[15 + t - 2 * k], a);
        a = __builtin_fmaf(R.wo[k], O[14 + t - 2 * k], a);
        b = __builtin_fmaf(R.wo[k], O[14 + t - 2 * k], b);
        b = __builtin_fmaf(R.we[k], E[15 + t - 2 * k], b);
      }
      ref[lane * 18 + t] = a;
      ref_swapped[lane * 18 + t] = b;
    }
    PD_WAVE_SYNC();
    ph_window_emit<true, true>(lane, *Le, R, 2, nullptr, pcm_emit);
    for (int s = 0; s < kHistSlots; s++) { hist_emit[s * 64 + lane] = R.he[s]; hist_emit[(kHistSlots + s) * 64 + lane] = R.ho[s]; }
  });
}
