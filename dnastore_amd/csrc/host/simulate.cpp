// dnas_simulate_reads_host: the statement of host/simulate.hpp as one loop over the positions of a strand, one thread, the entry
// state carried from position to position.  No ballots, no prefix sums.
#include "simulate.hpp"

#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "../errors.hpp"

namespace dnas {

int checkSimulateArgs(const dnas_mutator_params* params, int64_t n_strands, const int8_t* strand_seqs, const int64_t* strand_off,
                      int64_t n_reads, const int64_t* read_strand, double reverse_prob, int want_ops, int8_t** out_seqs,
                      int64_t** out_off, uint8_t** out_reversed, uint8_t** out_ops, int64_t** out_ops_off, const uint8_t* out_status) {
  if (out_seqs) *out_seqs = nullptr;
  if (out_off) *out_off = nullptr;
  if (out_reversed) *out_reversed = nullptr;
  if (out_ops) *out_ops = nullptr;
  if (out_ops_off) *out_ops_off = nullptr;
  if (!params || n_strands < 0 || n_reads < 0) return fail(DNAS_E_INVALID, "simulate reads: bad argument");
  if (!out_seqs || !out_off || !out_reversed || (want_ops && (!out_ops || !out_ops_off)))
    return fail(DNAS_E_INVALID, "simulate reads: null output argument");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kSimMaxLen) return fail(DNAS_E_UNSUPPORTED, "simulate reads: more than 32 duplication lengths");
  auto prob = [](double p) { return p >= 0 && p <= 1; };  // (false for a NaN)
  if (!prob(params->p_del_open) || !prob(params->p_del_extend) || !prob(params->p_tan_dup) || !prob(params->p_transition) ||
      !prob(params->p_transversion))
    return fail(DNAS_E_INVALID, "simulate reads: a probability of the error model is outside [0, 1]");
  for (int k = 0; k < params->n_len; ++k)
    if (!prob(params->p_len[k])) return fail(DNAS_E_INVALID, "simulate reads: pLen[" + std::to_string(k) + "] is outside [0, 1]");
  if (!(params->p_del_open + params->p_tan_dup <= 1)) return fail(DNAS_E_INVALID, "simulate reads: pDelOpen + pTanDup exceeds 1");
  if (!(params->p_transition + params->p_transversion <= 1)) return fail(DNAS_E_INVALID, "simulate reads: pTransition + pTransversion exceeds 1");
  if (!prob(reverse_prob)) return fail(DNAS_E_INVALID, "simulate reads: reverse_prob is outside [0, 1]");
  if (n_reads >= ((int64_t)1 << 31)) return fail(DNAS_E_UNSUPPORTED, "simulate reads: 2^31 reads or more in one call");
  if (n_strands > 0) {
    if (!strand_seqs || !strand_off) return fail(DNAS_E_INVALID, "simulate reads: null argument");
    if (strand_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
    for (int64_t s = 0; s < n_strands; ++s) {
      const int64_t I = strand_off[s + 1] - strand_off[s];
      if (I < 0) return fail(DNAS_E_INVALID, "strand " + std::to_string(s) + ": inconsistent offsets");
      if (I > kSimMaxStrand) return fail(DNAS_E_UNSUPPORTED, "strand " + std::to_string(s) + ": more than 2^20 bases");
    }
    int bad = 0;
    for (int64_t j = 0; j < strand_off[n_strands]; ++j) bad |= strand_seqs[j] & ~3;
    if (bad) return fail(DNAS_E_BAD_BASE, "bad base");
  }
  if (n_reads > 0) {
    if (!read_strand || !out_status) return fail(DNAS_E_INVALID, "simulate reads: null argument");
    for (int64_t r = 0; r < n_reads; ++r)
      if (read_strand[r] < 0 || read_strand[r] >= n_strands)
        return fail(DNAS_E_INVALID, "read " + std::to_string(r) + ": read_strand names no strand");
  }
  return DNAS_OK;
}

bool simulateReadHost(const SimThresholds& th, uint64_t seed, uint64_t index, const int8_t* in, int64_t I, std::vector<int8_t>* seq,
                      std::vector<uint8_t>* ops) {
  const size_t begin = seq->size();
  auto emit = [&](int base, uint8_t op) {
    if (base >= 0) seq->push_back((int8_t)base);
    if (ops) ops->push_back(op);
  };
  bool inDel = false;
  for (int64_t ip = 0; ip <= I; ++ip) {
    SimDraws d(seed, index, (uint32_t)ip);
    if (inDel && simExtend(th, d, ip, I)) {
      emit(-1, kSimOpDelete);
      continue;
    }
    inDel = simPosition(th, d, in, ip, I, emit);
  }
  SimDraws perRead(seed, index, kSimPerRead);
  const bool reversed = perRead.draw(0) < th.reverseProb;
  if (reversed) {
    for (size_t a = begin, b = seq->size(); a < b; ++a, --b) {
      const int8_t x = (*seq)[a], y = (*seq)[b - 1];
      (*seq)[a] = (int8_t)(3 - y);
      if (a != b - 1) (*seq)[b - 1] = (int8_t)(3 - x);
    }
  }
  return reversed;
}

namespace {
template <class T>
T* mallocCopy(const std::vector<T>& v, size_t n) {
  T* p = (T*)malloc((n ? n : 1) * sizeof(T));
  if (!p) throw std::bad_alloc();
  if (n) memcpy(p, v.data(), n * sizeof(T));
  return p;
}
}  // namespace

int simulateHandOut(int64_t n_reads, const std::vector<int8_t>& seqs, const std::vector<int64_t>& off, const std::vector<uint8_t>& reversed,
                    int want_ops, const std::vector<uint8_t>& ops, const std::vector<int64_t>& opsOff, int8_t** out_seqs, int64_t** out_off,
                    uint8_t** out_reversed, uint8_t** out_ops, int64_t** out_ops_off) {
  try {
    *out_seqs = mallocCopy(seqs, (size_t)off[(size_t)n_reads]);
    *out_off = mallocCopy(off, (size_t)n_reads + 1);
    *out_reversed = mallocCopy(reversed, (size_t)n_reads);
    if (want_ops) {
      *out_ops = mallocCopy(ops, (size_t)opsOff[(size_t)n_reads]);
      *out_ops_off = mallocCopy(opsOff, (size_t)n_reads + 1);
    }
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    free(*out_seqs), free(*out_off), free(*out_reversed);
    *out_seqs = nullptr, *out_off = nullptr, *out_reversed = nullptr;
    if (want_ops) {
      free(*out_ops), free(*out_ops_off);
      *out_ops = nullptr, *out_ops_off = nullptr;
    }
    return fail(DNAS_E_NOMEM, "out of memory");
  }
}

}  // namespace dnas
