// device_id = -1 (every GPU of the node): which devices, how independent work items are dealt over them, how a worker's share
// of the inputs is gathered, and the host thread per device.  Shared by every entry point that takes a device_id.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <new>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "errors.hpp"

namespace dnas {

// DNAS_OK when device_id names a device of this node or is -1, else the code, dnas_last_error set.
inline int checkDeviceId(int device_id) {
  const int have = dnas_device_count();
  if (have <= 0) return fail(DNAS_E_DEVICE, "no HIP device available");
  if (device_id < -1 || device_id >= have) return fail(DNAS_E_INVALID, "device_id out of range");
  return DNAS_OK;
}

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

// Shard `mine` of a concatenated array: its sequences one after the other, offsets from 0 (never an empty buffer: a null pointer
// is a bad argument).
template <class T>
void gatherShard(const std::vector<int64_t>& mine, const T* data, const int64_t* off, std::vector<T>* outData, std::vector<int64_t>* outOff) {
  outOff->assign(1, 0);
  for (int64_t i : mine) outOff->push_back(outOff->back() + off[i + 1] - off[i]);
  outData->resize(std::max<size_t>((size_t)outOff->back(), 1));
  for (size_t j = 0; j < mine.size(); ++j)
    std::copy(data + off[mine[j]], data + off[mine[j] + 1], outData->begin() + (*outOff)[j]);
}

// body(k) for every worker k, worker k on devices[k]: one host thread per worker (inline when there is one).  The first failure
// in worker order is returned, its message prefixed with the device (dnas_last_error is per thread).
template <class F>
int forEachDevice(const std::vector<int>& devices, F&& body) {
  const size_t W = devices.size();
  std::vector<int> rcs(W, DNAS_OK);
  std::vector<std::string> errs(W);
  auto run = [&](size_t k) {
    try {
      rcs[k] = body(k);
    } catch (const std::bad_alloc&) {
      rcs[k] = fail(DNAS_E_NOMEM, "out of memory");
    }
    if (rcs[k] != DNAS_OK) errs[k] = lastErrorSlot();
  };
  if (W == 1) {
    run(0);
  } else {
    std::vector<std::thread> workers;
    for (size_t k = 0; k < W; ++k) workers.emplace_back(run, k);
    for (auto& t : workers) t.join();
  }
  for (size_t k = 0; k < W; ++k)
    if (rcs[k] != DNAS_OK) return fail(rcs[k], "device " + std::to_string(devices[k]) + ": " + errs[k]);
  return DNAS_OK;
}

}  // namespace dnas
