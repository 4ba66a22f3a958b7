// mfcc_core.h -- what k_clip_mfcc (mfcc.hip) adds to mel_core.h's and fbank_core.h's indexing and
// arithmetic: the floats a frame takes in the LDS region the powers and then the cepstra share, the column the energy goes
// to, and one output value.  One source for the kernel and for the host build the tests compile with g++
// (tests/host_emul/mfcc_emul.cpp).
#ifndef PDMP3_MFCC_CORE_H
#define PDMP3_MFCC_CORE_H
#include "fbank_core.h"

namespace pdmp3 {

// the cepstra of a frame lie ceps16 + 1 floats apart (the spare float holds the frame's energy), its powers bins16 + 2
MEL_FN int mfcc_ceps_stride(int ceps16) { return ceps16 + 1; }
// floats of the second LDS region: first the powers [tile][bins16 + 2], then the cepstra [tile][ceps16 + 1] in their place
MEL_FN unsigned mfcc_second_region(int tile, int bins16, int ceps16) {
  const int a = bins16 + 2, b = mfcc_ceps_stride(ceps16);
  return (unsigned)tile * (unsigned)(a > b ? a : b);
}
// the column the energy replaces C0 in: 0, or the last with htk_compat; -1 without use_energy
MEL_FN int mfcc_energy_column(int n_ceps, int use_energy, int htk_compat) {
  if (!use_energy) return -1;
  return htk_compat ? n_ceps - 1 : 0;
}
// column dc of a frame whose cepstra start at `ceps` (the energy E behind them, at ceps[ceps16]): the folded table's product
// as it is (lifter, sqrt 2 and column order are in the table), or the energy column's value
MEL_FN float mfcc_output(const float* ceps, int ceps16, int dc, int energy_column, float eps, float log_floor) {
  if (dc == energy_column) return fbank_energy_output(ceps[ceps16], eps, log_floor, 1);
  return ceps[dc];
}

}  // namespace pdmp3
#endif
