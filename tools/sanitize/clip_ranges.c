/* Sanitizer driver (tools/sanitize/run.sh): stream indices with and without snapshots, and the host hook's frame ranges
 * (pdmp3_amd_bulk_parse_range), against the whole stream's records -- the index, halo rule and range scan of clip.c under
 * ASan / UBSan / TSan on the CPU build.  Prints the ranges checked and how many differed (0). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "pdmp3_bulk.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s file.mp3\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const size_t n = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  unsigned char* mp3 = (unsigned char*)malloc(n);
  if (!mp3 || fread(mp3, 1, n, f) != n) return 2;
  fclose(f);
  long long frames = 0;
  if (pdmp3_amd_scan_buffer(mp3, n, &frames) < 0 || frames < 2) return 2;
  const size_t cap = (size_t)frames + 1;
  int16_t* sp = (int16_t*)malloc(cap * 2304 * sizeof(int16_t));
  pdmp3_gc_side* sd = (pdmp3_gc_side*)malloc(cap * 4 * sizeof(pdmp3_gc_side));
  int16_t* rsp = (int16_t*)malloc(cap * 2304 * sizeof(int16_t));
  pdmp3_gc_side* rsd = (pdmp3_gc_side*)malloc(cap * 4 * sizeof(pdmp3_gc_side));
  pdmp3_amd_bulk* b = pdmp3_amd_bulk_new_parse_only(4, 64);
  long long pcm = 0;
  if (!sp || !sd || !rsp || !rsd || !b || pdmp3_amd_bulk_parse(b, mp3, n, sp, sd, cap, &pcm) != frames) return 1;
  int bad = 0, checked = 0;
  for (int spacing = 16; spacing <= 1 << 20; spacing *= 64) {
    pdmp3_amd_index* ix = pdmp3_amd_index_new_spacing(mp3, n, 0, spacing);
    if (!ix || pdmp3_amd_index_frames(ix) != frames || pdmp3_amd_index_pcm_offset(ix, frames) != pcm) return 1;
    srand(7);
    for (int t = 0; t < 40; t++) {
      const long long a = rand() % frames, c = 1 + rand() % 300;
      long long f0 = -1;
      const long long got = pdmp3_amd_bulk_parse_range(b, mp3, n, ix, a, c, 1, rsp, rsd, cap, &f0);
      const long long e = a + c < frames ? a + c : frames;
      if (got != e - f0 || f0 < 0 || f0 > a) { bad++; continue; }
      /* frames [a, e): records and spectra as in the whole parse */
      if (memcmp(rsp + (a - f0) * 2304, sp + a * 2304, (size_t)(e - a) * 2304 * sizeof(int16_t)) ||
          memcmp(rsd + (a - f0) * 4, sd + a * 4, (size_t)(e - a) * 4 * sizeof(pdmp3_gc_side)))
        bad++;
      checked++;
    }
    printf("spacing %d: split %d\n", spacing, pdmp3_amd_index_split(ix));
    pdmp3_amd_index_delete(ix);
  }
  pdmp3_amd_bulk_delete(b);
  free(sp); free(sd); free(rsp); free(rsd); free(mp3);
  printf("clip_ranges: %d ranges, %d differ\n", checked, bad);
  return bad != 0;
}
