// device_id = -1 (every GPU of the node): which devices, and how independent work items are dealt over them.
// Shared by dnas_decode_fastseqs_ex (reads, by length) and the E-step handle (alignment pairs, by inLen + outLen).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <vector>

#include "../../include/dnastore_amd.h"

namespace dnas {

// device_id >= 0: that device.  Negative: every visible GPU; DNAS_FAKE_DEVICES=n makes it n workers on devices d % have
// (tests: several host threads share the GPUs there are).  Empty when no GPU is visible.
inline std::vector<int> pickDevices(int device_id) {
  if (device_id >= 0) return {device_id};
  std::vector<int> devices;
  const int have = dnas_device_count();
  if (have <= 0) return devices;
  int use = have;
  if (const char* s = getenv("DNAS_FAKE_DEVICES")) use = std::max(1, atoi(s));
  for (int d = 0; d < use; ++d) devices.push_back(d % have);
  return devices;
}

// Item i costs cost[i]: deal the items over W workers, costliest first, in snake order (0..W-1, W-1..0, ...; what
// shard.partition does for the one-process-per-GPU bench).  Each worker's list is in ascending item order.
inline std::vector<std::vector<int64_t>> snakeDeal(const std::vector<int64_t>& cost, size_t W) {
  std::vector<int64_t> order(cost.size());
  std::iota(order.begin(), order.end(), (int64_t)0);
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return cost[(size_t)a] > cost[(size_t)b]; });
  std::vector<std::vector<int64_t>> shard(W);
  for (size_t pos = 0; pos < order.size(); ++pos) {
    const size_t round = pos / W, k = pos % W;
    shard[round % 2 == 0 ? k : W - 1 - k].push_back(order[pos]);
  }
  for (auto& sh : shard) std::sort(sh.begin(), sh.end());
  return shard;
}

}  // namespace dnas
