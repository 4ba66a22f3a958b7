// The granule kernel's routing word (pdmp3_amd/csrc/decode_core.h: GranRoute, gran_route_offset, gran_route_pred) against the
// expressions run_granule_wave, run_granule and frame_is_rare decided from before the word existed -- kept here verbatim, on
// the same records.  A stand-alone program: every combination of
//   mode (4) x mode_extension bit 0 x RESET x lsf version bits (4), for each of the frames f - 1, f, f + 1
//   x the H5 flag of record (f, 1, 1) x gr x f first, middle or last of the launch x a state block or none
// (the first and last positions also as a launch of ONE frame).  Prints the number of cases and exits 0 when all agree.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../pdmp3_amd/csrc/decode_core.h"

using namespace pdmp3;

namespace {

// ---- the expressions of before, verbatim (DecodeArgs a; granule g) ----------------------------------------------------
bool old_frame_is_rare(const pdmp3_gc_side* rec) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(rec);
  const unsigned fr = b[7];
  const bool is = ((fr & PDMP3_FR_MODE_MASK) >> PDMP3_FR_MODE_SHIFT) == 1 && (fr & (1u << PDMP3_FR_MODEEXT_SHIFT));
  return is || (b[offsetof(pdmp3_gc_side, lsf)] & PDMP3_LSF_VERSION_MASK) != 0;
}

struct Facts {
  bool stereo, fresh, prev_stereo, rare, prev_rare, next_rare, h5, next_takes, from_caller, h5_tail_from_caller;
  bool operator==(const Facts& o) const {
    return stereo == o.stereo && fresh == o.fresh && prev_stereo == o.prev_stereo && rare == o.rare && prev_rare == o.prev_rare &&
           next_rare == o.next_rare && h5 == o.h5 && next_takes == o.next_takes && from_caller == o.from_caller &&
           h5_tail_from_caller == o.h5_tail_from_caller;
  }
};

Facts old_facts(const DecodeArgs& a, int g) {
  const int f = g >> 1, gr = g & 1;
  const uint8_t fb = reinterpret_cast<const uint8_t*>(a.side + (size_t)f * 4)[7];
  const uint8_t pb = reinterpret_cast<const uint8_t*>(a.side + (size_t)(f > 0 ? f - 1 : 0) * 4)[7];
  const uint8_t nb = reinterpret_cast<const uint8_t*>(a.side + (size_t)(f + 1 < a.n_frames ? f + 1 : f) * 4)[7];
  const uint8_t fl = reinterpret_cast<const uint8_t*>(a.side + (size_t)(2 * f + 1) * 2 + 1)[3];
  const bool rare = old_frame_is_rare(a.side + (size_t)f * 4);
  const bool prev_rare = old_frame_is_rare(a.side + (size_t)(f > 0 ? f - 1 : 0) * 4);
  const bool next_rare = old_frame_is_rare(a.side + (size_t)(f + 1 < a.n_frames ? f + 1 : f) * 4);
  const bool stereo = ((fb & PDMP3_FR_MODE_MASK) >> PDMP3_FR_MODE_SHIFT) != 3 && !rare;
  const bool fresh = f == 0 || (fb & PDMP3_FR_RESET);       // its input state is the caller's / zero
  const bool prev_stereo = ((pb & PDMP3_FR_MODE_MASK) >> PDMP3_FR_MODE_SHIFT) != 3 && !prev_rare;
  const bool h5 = (fl & PDMP3_GC_WIN_SWITCH) && ((fl & PDMP3_GC_BLOCK_TYPE_MASK) >> PDMP3_GC_BLOCK_TYPE_SHIFT) == 2;
  // (run_granule_wave sets next_takes on chained frames only; the expression itself is compared on all)
  const bool next_takes = gr == 0 || (f + 1 < a.n_frames && ((nb & PDMP3_FR_MODE_MASK) >> PDMP3_FR_MODE_SHIFT) != 3 && !(nb & PDMP3_FR_RESET) && !next_rare);
  // run_granule
  const bool from_caller = fresh && gr == 0 && f == 0 && a.state_in && !(reinterpret_cast<const uint8_t*>(a.side)[7] & PDMP3_FR_RESET);
  const bool h5_tail = fresh && f == 0 && a.state_in && !(reinterpret_cast<const uint8_t*>(a.side)[7] & PDMP3_FR_RESET);
  return Facts{stereo, fresh, prev_stereo, rare, prev_rare, next_rare, h5, next_takes, from_caller, h5_tail};
}

// ---- the word: every lane's byte and predicate, as the wave's load and ballot form it ---------------------------------
Facts new_facts(const DecodeArgs& a, int g) {
  const int f = g >> 1, gr = g & 1;
  unsigned long long ballot = 0;
  for (int lane = 0; lane < 64; lane++) {              // (every lane of the wave loads: none may leave the records)
    const size_t off = gran_route_offset(lane, f, a.n_frames);
    if (off >= (size_t)a.n_frames * 4 * sizeof(pdmp3_gc_side)) { fprintf(stderr, "lane %d reads past the records\n", lane); exit(2); }
    const unsigned b = reinterpret_cast<const uint8_t*>(a.side)[off];
    if (gran_route_pred(lane, b)) ballot |= 1ull << lane;
  }
  const GranRoute route{(unsigned)ballot};
  const bool fresh = f == 0 || route.reset(0);
  const bool next_takes = gr == 0 || (f + 1 < a.n_frames && route.takes_chain(2));
  const bool from_caller = fresh && gr == 0 && f == 0 && a.state_in && !route.reset(0);
  const bool h5_tail = fresh && f == 0 && a.state_in && !route.reset(0);
  return Facts{route.stereo(0), fresh, route.stereo(1), route.rare(0), route.rare(1), route.rare(2), route.h5(), next_takes, from_caller, h5_tail};
}

// a frame's four records from its case number: mode (2 bits) | mode_ext bit 0 | RESET | lsf version bits (2)
constexpr int kFrameCases = 4 * 2 * 2 * 4;
void set_frame(pdmp3_gc_side* rec, int c, unsigned noise) {
  const unsigned mode = c & 3, ext0 = (c >> 2) & 1, reset = (c >> 3) & 1, ver = (c >> 4) & 3;
  // (the bits nobody decides from -- sampling frequency, mode_extension bit 1, bit 7; the lsf byte's other bits -- vary too)
  const uint8_t fr = (uint8_t)((noise & PDMP3_FR_SFREQ_MASK) | (mode << PDMP3_FR_MODE_SHIFT) | (ext0 << PDMP3_FR_MODEEXT_SHIFT) |
                               (((noise >> 2) & 1) << (PDMP3_FR_MODEEXT_SHIFT + 1)) | (reset ? PDMP3_FR_RESET : 0));
  for (int r = 0; r < 4; r++) {
    rec[r].frame = fr;
    rec[r].lsf = (uint8_t)(ver | (((noise >> 3) & 1) ? PDMP3_LSF_IS_SCALE : 0));
  }
}

}  // namespace

int main() {
  static_assert(offsetof(pdmp3_gc_side, frame) == 7 && offsetof(pdmp3_gc_side, flags) == 3, "the bytes the kernel reads");
  float state_block[4] = {0, 0, 0, 0};
  long cases = 0, bad = 0;
  // position: 0 first of three, 1 middle of three, 2 last of three, 3 the only frame
  for (int pos = 0; pos < 4; pos++) {
    const int n = pos == 3 ? 1 : 3, f = pos == 3 ? 0 : pos;
    std::vector<pdmp3_gc_side> side((size_t)n * 4);
    for (auto& r : side) memset(&r, 0, sizeof r);
    DecodeArgs a;
    memset(&a, 0, sizeof a);
    a.side = side.data();
    a.n_frames = n;
    // the frames around f that exist; a frame that does not exist has one case
    const int nc_prev = f > 0 ? kFrameCases : 1, nc_next = f + 1 < n ? kFrameCases : 1;
    for (int cf = 0; cf < kFrameCases; cf++)
      for (int cp = 0; cp < nc_prev; cp++)
        for (int cn = 0; cn < nc_next; cn++) {
          const unsigned noise = (unsigned)(cf * 7 + cp * 3 + cn);
          set_frame(&side[(size_t)f * 4], cf, noise);
          if (f > 0) set_frame(&side[(size_t)(f - 1) * 4], cp, noise >> 1);
          if (f + 1 < n) set_frame(&side[(size_t)(f + 1) * 4], cn, noise >> 2);
          // the flags byte of (f, 1, 1): H5 or not in the full product; all 256 values of the byte where the frames around f
          // are the first case
          const int n_fl = (cp == 0 && cn == 0) ? 256 : 2;
          for (int fl = 0; fl < n_fl; fl++) {
            side[(size_t)f * 4 + 3].flags = n_fl == 2 ? (uint8_t)(fl ? (PDMP3_GC_WIN_SWITCH | (2u << PDMP3_GC_BLOCK_TYPE_SHIFT)) : 0) : (uint8_t)fl;
            // (the other records' flags are not read: set to what would mislead)
            for (int r = 0; r < 3; r++) side[(size_t)f * 4 + r].flags = (uint8_t)~side[(size_t)f * 4 + 3].flags;
            for (int gr = 0; gr < 2; gr++)
              for (int st = 0; st < 2; st++) {
                a.state_in = st ? state_block : nullptr;
                const Facts o = old_facts(a, 2 * f + gr), w = new_facts(a, 2 * f + gr);
                cases++;
                if (!(o == w)) {
                  if (bad++ < 10)
                    fprintf(stderr, "pos %d frame case %d prev %d next %d flags %02x gr %d state %d: old %d%d%d%d%d%d%d%d%d%d new %d%d%d%d%d%d%d%d%d%d\n", pos, cf, cp, cn,
                            side[(size_t)f * 4 + 3].flags, gr, st, o.stereo, o.fresh, o.prev_stereo, o.rare, o.prev_rare, o.next_rare, o.h5, o.next_takes,
                            o.from_caller, o.h5_tail_from_caller, w.stereo, w.fresh, w.prev_stereo, w.rare, w.prev_rare, w.next_rare, w.h5, w.next_takes,
                            w.from_caller, w.h5_tail_from_caller);
                }
              }
          }
        }
  }
  printf("cases %ld mismatches %ld\n", cases, bad);
  return bad ? 1 : 0;
}
