// Stand-alone host program around csrc/label_class.h (tests/test_dataset_conversion_cpu.py builds it with the address and
// undefined-behaviour sanitizers): label_class_host <dtype> <in.bin> <out.bin> reads the raw values of that type into an exact-size
// buffer and writes, per value, the slot (int32) followed by all keys (uint64) of mt_label_slot / mt_label_key.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "label_class.h"

template <typename T> static int run(const char* in, const char* out) {
  FILE* f = fopen(in, "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)bytes / sizeof(T));
  if (fread(v.data(), sizeof(T), v.size(), f) != v.size()) return 3;
  fclose(f);
  std::vector<int32_t> slot(v.size());
  std::vector<uint64_t> key(v.size());
  for (size_t i = 0; i < v.size(); ++i) { slot[i] = mt_label_slot(v[i]); key[i] = mt_label_key(v[i]); }
  f = fopen(out, "wb");
  if (!f) return 4;
  fwrite(slot.data(), sizeof(int32_t), slot.size(), f);
  fwrite(key.data(), sizeof(uint64_t), key.size(), f);
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 4) return 1;
  const char* t = argv[1];
  if (!strcmp(t, "uint8")) return run<uint8_t>(argv[2], argv[3]);
  if (!strcmp(t, "int8")) return run<int8_t>(argv[2], argv[3]);
  if (!strcmp(t, "int16")) return run<int16_t>(argv[2], argv[3]);
  if (!strcmp(t, "uint16")) return run<uint16_t>(argv[2], argv[3]);
  if (!strcmp(t, "int32")) return run<int32_t>(argv[2], argv[3]);
  if (!strcmp(t, "uint32")) return run<uint32_t>(argv[2], argv[3]);
  if (!strcmp(t, "float32")) return run<float>(argv[2], argv[3]);
  if (!strcmp(t, "float64")) return run<double>(argv[2], argv[3]);
  return 1;
}
