// Host check of the patch gather's index and pad arithmetic (multitalent_amd/csrc/patch_index.h, the function the device kernel
// compiles): gathers a patch out of a synthetic case into heap buffers of EXACTLY the needed size, so that the address and
// undefined-behaviour sanitizers this program is built with see any index outside the source or the patch.
//   patch_gather_host C sx sy sz lbx lby lbz PD PH PW pad_mode out_file
// case: data[c][i] = c * 100000 + i, seg[i] = i % 7 - 1 (int16).  out_file: float32 data [C, PD, PH, PW], then seg [PD, PH, PW].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "patch_index.h"

int main(int argc, char** argv) {
  if (argc != 13) return 2;
  const int C = atoi(argv[1]);
  const int shape[3] = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
  const int lb[3] = {atoi(argv[5]), atoi(argv[6]), atoi(argv[7])};
  const int PD = atoi(argv[8]), PH = atoi(argv[9]), PW = atoi(argv[10]), pad_mode = atoi(argv[11]);
  const long V = (long)shape[0] * shape[1] * shape[2], PV = (long)PD * PH * PW;
  float* data = new float[C * V];
  int16_t* seg = new int16_t[V];
  float* data_out = new float[C * PV];
  float* seg_out = new float[PV];
  for (int c = 0; c < C; ++c)
    for (long i = 0; i < V; ++i) data[c * V + i] = (float)(c * 100000 + i);
  for (long i = 0; i < V; ++i) seg[i] = (int16_t)(i % 7 - 1);
  for (int d = 0; d < PD; ++d)
    for (int h = 0; h < PH; ++h)
      for (int w = 0; w < PW; ++w) {
        const long o = ((long)d * PH + h) * PW + w;
        const long s = mt_patch_source(shape, lb, d, h, w, pad_mode);
        for (int c = 0; c < C; ++c) data_out[c * PV + o] = s >= 0 ? data[c * V + s] : 0.f;
        const long t = mt_patch_source(shape, lb, d, h, w, 0);
        seg_out[o] = t >= 0 ? (float)seg[t] : -1.f;
      }
  FILE* f = fopen(argv[12], "wb");
  if (!f) return 3;
  const bool ok = fwrite(data_out, sizeof(float), C * PV, f) == (size_t)(C * PV) && fwrite(seg_out, sizeof(float), PV, f) == (size_t)PV;
  fclose(f);
  delete[] data; delete[] seg; delete[] data_out; delete[] seg_out;
  return ok ? 0 : 4;
}
