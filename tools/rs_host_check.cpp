// The host side of the outer code -- the statement (csrc/host/rs.cpp: long division, the solver of rs.hpp, which is also the text
// rs_solve_kernel runs) and the file layer (csrc/host/outer.cpp, host = 1) -- in a program of its own, for AddressSanitizer and
// UBSan: columns from clean to far beyond capacity on eight codes, a pool of records with lost, short, long and damaged ones.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o rs_host_check tools/rs_host_check.cpp dnastore_amd/csrc/host/rs.cpp \
//       dnastore_amd/csrc/host/outer.cpp
// The two device entries the file layer can call are stubs here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "../include/dnastore_amd.h"
#include "../dnastore_amd/csrc/errors.hpp"
namespace dnas { std::string& lastErrorSlot() { static thread_local std::string s; return s; } }
extern "C" int dnas_rs_encode(int32_t, int32_t, int32_t, int64_t, const uint8_t*, uint8_t*, dnas_rs_stats*, int) { return -7; }
extern "C" int dnas_rs_decode(int32_t, int32_t, int32_t, int64_t, const uint8_t*, const uint8_t*, uint8_t*, uint8_t*, uint8_t*, int32_t*, dnas_rs_stats*, int) { return -7; }
int main() {
  std::mt19937 rng(1);
  const int codes[][2] = {{2,1},{3,2},{8,2},{64,33},{65,1},{129,128},{255,191},{255,223}};
  long cols = 0, st[3] = {0,0,0};
  for (auto& c : codes) {
    const int n = c[0], k = c[1], r = n - k, L = 7, B = 12;
    std::vector<uint8_t> data(B*k*L), blocks(B*n*L), out(B*n*L), present(B*n), status(B*L), errors(B*L);
    std::vector<int32_t> fixed(B*n);
    for (auto& x : data) x = rng();
    if (dnas_rs_encode_host(n, k, L, B, data.data(), blocks.data())) return 1;
    for (int b = 0; b < B; ++b) {
      const int f = b % (r + 2) > n ? n : b % (r + 2);
      for (int p = 0; p < n; ++p) present[b*n+p] = 1;
      for (int q = 0; q < f; ++q) present[b*n + rng() % n] = 0;
      for (int j = 0; j < L; ++j) for (int e = 0; e < (j % (r/2 + 3)); ++e) blocks[(b*n + rng() % n)*L + j] ^= 1 + rng() % 255;
    }
    if (dnas_rs_decode_host(n, k, L, B, blocks.data(), present.data(), out.data(), status.data(), errors.data(), fixed.data())) return 2;
    for (auto s : status) { ++st[s]; ++cols; }
  }
  // the file layer
  std::vector<uint8_t> file(777);
  for (auto& x : file) x = rng();
  int64_t B = 0; uint8_t* rec = nullptr;
  if (dnas_outer_encode(file.data(), file.size(), 12, 8, 10, 0, 1, &B, &rec)) return 3;
  std::vector<uint8_t> bytes; std::vector<int64_t> off{0}; std::vector<double> w;
  for (int64_t s = 0; s < B*12; ++s) {
    if (s % 12 == 3 || s % 12 == 7) continue;
    int len = 14; if (s % 17 == 0) len = 9; if (s % 19 == 0) len = 20;
    for (int i = 0; i < len; ++i) bytes.push_back(i < 14 ? rec[s*14 + i] : 0);
    if (s % 23 == 0) bytes.back() ^= 1;
    off.push_back(bytes.size()); w.push_back(1 + s % 3);
  }
  std::vector<uint8_t> present(B*12), col(B*10); std::vector<int32_t> fixed(B*12);
  uint8_t* data = nullptr; int64_t len = 0, nr = 0, *ranges = nullptr; int32_t status = 0; dnas_outer_stats os;
  if (dnas_outer_decode(off.size()-1, bytes.data(), off.data(), w.data(), 12, 8, 10, B, 0, 1, &data, &len, &status, present.data(), col.data(), fixed.data(), &ranges, &nr, &os)) { printf("%s\n", dnas_last_error()); return 4; }
  printf("columns %ld ok %ld corrected %ld failed %ld; outer status %d len %ld ranges %ld dropped %ld erased %ld same %d\n", cols, st[0], st[1], st[2], status, (long)len, (long)nr, (long)os.dropped, (long)os.erased, len == 777 && !memcmp(data, file.data(), 777));
  dnas_free(data); dnas_free(ranges);
  // the whole pool, last record first: the file
  bytes.clear(); off.assign(1, 0);
  for (int64_t s = B*12 - 1; s >= 0; --s) { bytes.insert(bytes.end(), rec + s*14, rec + s*14 + 14); off.push_back(bytes.size()); }
  if (dnas_outer_decode(off.size()-1, bytes.data(), off.data(), nullptr, 12, 8, 10, B, 0, 1, &data, &len, &status, present.data(), col.data(), fixed.data(), &ranges, &nr, &os)) return 5;
  const bool whole = status == DNAS_OUTER_OK && len == 777 && !memcmp(data, file.data(), 777) && nr == 0 && os.erased == 0;
  dnas_free(data); dnas_free(ranges); dnas_free(rec);
  if (!whole || st[0] == 0 || st[1] == 0 || st[2] == 0) return 6;
  printf("rs host check: ok\n");
  return 0;
}
extern "C" const char* dnas_last_error(void) { return dnas::lastErrorSlot().c_str(); }
extern "C" void dnas_free(void* p) { free(p); }
