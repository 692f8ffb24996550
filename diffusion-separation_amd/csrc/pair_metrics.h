// pair_metrics.h — the calling convention that the on-device measures on pairs share (stoi.hip, composite.hip): a zero-padded
// batch ref / est [B][S][T] fp32, pair = (utterance b, reference row i, estimate row perm[b][i]), lengths[b] clamped to [0, T];
// results in float64, scratch in a caller-owned workspace, tables built once per device.  ONE definition of the addressing and
// of the boundary checks; the measures themselves (framing, spectra, windows) stay in their own files.
#pragma once

#include <map>
#include <mutex>
#include <vector>

#include "common.h"

namespace {

// ---------------------------------------------------------------- device side
// samples of utterance b that count (lengths null: all T)
__device__ inline int ds_pair_len(const int* lengths, int b, long T) {
  long n = lengths ? (long)lengths[b] : T;
  return (int)(n < 0 ? 0 : (n > T ? T : n));
}
// row of signal sig (0 reference, 1 estimate) of a pair; a perm entry outside [0, S) is clamped, never followed
__device__ inline const float* ds_pair_row(const float* ref, const float* est, const int* perm, int pair, int sig, int S, long T) {
  const int b = pair / S;
  int row = pair % S;
  if (sig == 1 && perm) {
    row = perm[pair];
    row = row < 0 ? 0 : (row >= S ? S - 1 : row);
  }
  return (sig == 0 ? ref : est) + ((long)b * S + row) * T;
}

// ---------------------------------------------------------------- host side
// Carves a workspace into 256-byte aligned pieces: take(bytes) returns the piece's offset, total is what the caller must bring.
struct DsCarver {
  int64_t total = 0;
  int64_t take(int64_t bytes) {
    const int64_t off = total;
    total += (bytes + 255) / 256 * 256;
    return off;
  }
};

// A table of doubles that lives on the device for the rest of the process, one per (current device, key): build(table, extra)
// fills it on the host the first time, with a small host struct that is kept with it (DsNoExtra: none).  Each call site has a
// cache of its own (the statics of this instantiation).
struct DsNoExtra {};
template <typename Extra, typename Build>
int ds_device_table(std::pair<int, int> key, Build build, const double** out, Extra* extra) {
  struct Entry { double* dev; Extra extra; };
  static std::mutex mu;
  static std::map<std::pair<int, std::pair<int, int>>, Entry> cache;
  int dev = 0;
  DS_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> g(mu);
  auto it = cache.find({dev, key});
  if (it == cache.end()) {
    std::vector<double> t;
    Entry e{};
    build(t, e.extra);
    DS_HIP(hipMalloc(&e.dev, t.size() * sizeof(double)));
    DS_HIP(hipMemcpy(e.dev, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice));
    it = cache.insert({{dev, key}, e}).first;
  }
  *out = it->second.dev;
  *extra = it->second.extra;
  return 0;
}

// The boundary checks of an entry `name` once its layout is known: P pairs, a workspace of `need` bytes.
inline int ds_pair_check(const std::string& name, const void* ref, const void* est, const void* out, const void* workspace,
                         int64_t workspace_bytes, int64_t P, int64_t need) {
  DS_CHECK(ref && est && out && workspace, name + ": null pointer");
  DS_CHECK(P <= 65535, name + ": more than 65535 (utterance, source) pairs in one call");
  DS_CHECK(workspace_bytes >= need, name + ": workspace too small (" + std::to_string(workspace_bytes) + " < " + std::to_string(need) + " bytes)");
  DS_CHECK(((uintptr_t)workspace & 7) == 0, name + ": workspace must be 8-byte aligned");
  return 0;
}

}  // namespace
