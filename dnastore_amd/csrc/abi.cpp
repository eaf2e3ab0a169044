// Host-only half of the C ABI (include/dnastore_amd.h): file formats, flattening and the
// decodeFastSeqs convenience call.  The device half lives in runtime.hip.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/dnastore_amd.h"
#include "devices.hpp"
#include "errors.hpp"
#include "host/decoder.hpp"
#include "host/encoder.hpp"
#include "host/fastseq.hpp"
#include "host/machine.hpp"
#include "host/model.hpp"
#include "host/assign.hpp"
#include "host/cluster.hpp"
#include "host/consensus.hpp"
#include "host/pairalign.hpp"
#include "host/baumwelch.hpp"
#include "host/paircounts.hpp"
#include "host/pairforward.hpp"
#include "host/polish.hpp"
#include "host/stockholm.hpp"
#include "host/simulate.hpp"
#include "host/trim.hpp"

struct dnas_machine { dnas::Machine machine; };
struct dnas_flat { dnas::FlatModel flat; };
struct dnas_fastseqs { std::vector<dnas::FastSeq> seqs; };
struct dnas_pairs { dnas::AlignmentPairs db; dnas_pairs_view view; };
struct dnas_decoded {
  std::vector<dnas::FastSeq> seqs;
  std::vector<double> loglike;
  std::vector<std::vector<uint64_t>> events;   // per read, when asked for
  std::string tier;                            // which fill kernel served the machine
  int devices = 1;
  std::vector<uint8_t> strand;                 // per read: 1 = decoded from its reverse complement
};

namespace dnas {
std::string& lastErrorSlot() {
  thread_local std::string slot;
  return slot;
}
}  // namespace dnas

namespace {

// Map the host layer's exceptions to ABI status codes (reference behaviour in comments).
template <class F>
int guarded(F&& body) {
  try {
    return body();
  } catch (const std::domain_error& e) {  // cyclic null graph, trans.cpp:631-632
    return dnas::fail(DNAS_E_CYCLIC, e.what());
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    const std::string w = e.what();
    int code = DNAS_E_PARSE;
    if (w.rfind("File not found", 0) == 0 || w.rfind("Couldn't open", 0) == 0) code = DNAS_E_IO;  // Fail -> exit(1)
    else if (w.rfind("Not a DNA-outputting machine", 0) == 0) code = DNAS_E_NOT_DNA;
    else if (w.rfind("Unknown symbol", 0) == 0) code = DNAS_E_BAD_BASE;
    else if (w.rfind("pLen longer than", 0) == 0) code = DNAS_E_UNSUPPORTED;  // as dnas_model_create_ex says it
    return dnas::fail(code, w);
  }
}

}  // namespace

extern "C" {

const char* dnas_last_error(void) { return dnas::lastErrorSlot().c_str(); }
void dnas_free(void* p) { free(p); }

int dnas_machine_load_json(const char* path, dnas_machine** out) {
  if (!path || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    *out = new dnas_machine{dnas::Machine::fromFile(path)};
    return DNAS_OK;
  });
}

int dnas_machine_parse_json(const char* text, size_t len, dnas_machine** out) {
  if (!text || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    *out = new dnas_machine{dnas::Machine::fromJSON(std::string(text, len))};
    return DNAS_OK;
  });
}

void dnas_machine_free(dnas_machine* m) { delete m; }
int32_t dnas_machine_n_states(const dnas_machine* m) { return m ? (int32_t)m->machine.nStates() : 0; }

int dnas_machine_write_json(const dnas_machine* m, char** out_text, size_t* out_len) {
  if (!m || !out_text || !out_len) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    std::ostringstream ss;
    m->machine.writeJSON(ss);
    const std::string s = ss.str();
    char* buf = (char*)malloc(s.size() + 1);
    if (!buf) throw std::bad_alloc();
    memcpy(buf, s.c_str(), s.size() + 1);
    *out_text = buf;
    *out_len = s.size();
    return DNAS_OK;
  });
}

static int encoded_to_c(dnas::Encoder& enc, char** out_dna, size_t* out_len) {
  enc.close();
  const std::string& s = enc.output();
  char* buf = (char*)malloc(s.size() + 1);
  if (!buf) throw std::bad_alloc();
  memcpy(buf, s.c_str(), s.size() + 1);
  *out_dna = buf;
  *out_len = s.size();
  return DNAS_OK;
}

int dnas_encode_symbols(const dnas_machine* m, const char* symbols, size_t n, char** out_dna, size_t* out_len) {
  if (!m || (!symbols && n) || !out_dna || !out_len) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    dnas::Encoder enc(m->machine);
    enc.encodeSymbolString(std::string(symbols, n));
    return encoded_to_c(enc, out_dna, out_len);
  });
}

int dnas_encode_bytes(const dnas_machine* m, const uint8_t* bytes, size_t n, char** out_dna, size_t* out_len) {
  if (!m || (!bytes && n) || !out_dna || !out_len) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    dnas::Encoder enc(m->machine);
    enc.encodeBytes(std::string((const char*)bytes, n));
    return encoded_to_c(enc, out_dna, out_len);
  });
}

int dnas_machine_compose(const dnas_machine* first, const dnas_machine* second, dnas_machine** out) {
  if (!first || !second || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    *out = new dnas_machine{dnas::Machine::compose(first->machine, second->machine)};
    return DNAS_OK;
  });
}

int dnas_decode_exact(const dnas_machine* m, const char* dna, size_t n, char** out_symbols, size_t* out_len) {
  if (!m || (!dna && n) || !out_symbols || !out_len) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    dnas::Decoder dec(m->machine);
    dec.decodeString(std::string(dna, n));
    dec.close();
    const std::string& s = dec.symbols();
    char* buf = (char*)malloc(s.size() + 1);
    if (!buf) throw std::bad_alloc();
    memcpy(buf, s.c_str(), s.size() + 1);
    *out_symbols = buf;
    *out_len = s.size();
    return DNAS_OK;
  });
}

int dnas_symbols_to_bytes(const char* symbols, size_t n, uint8_t** out_bytes, size_t* out_len) {
  if ((!symbols && n) || !out_bytes || !out_len) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    const std::string b = dnas::symbolsToBytes(std::string(symbols, n));
    uint8_t* buf = (uint8_t*)malloc(b.size() + 1);
    if (!buf) throw std::bad_alloc();
    memcpy(buf, b.data(), b.size());
    *out_bytes = buf;
    *out_len = b.size();
    return DNAS_OK;
  });
}

int dnas_mutator_params_from_flags(double sub_prob, double iv_ratio, double dup_prob, double del_open, double del_ext,
                                   int global, int length, dnas_mutator_params* out) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    dnas::MutatorParams::fromFlags(sub_prob, iv_ratio, dup_prob, del_open, del_ext, global != 0, length).toC(out);
    return DNAS_OK;
  });
}

int dnas_mutator_params_load_json(const char* path, dnas_mutator_params* out) {
  if (!path || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    dnas::MutatorParams::fromFile(path).toC(out);
    return DNAS_OK;
  });
}

int dnas_flatten(const dnas_machine* m, const dnas_mutator_params* p, dnas_flat** out) {
  if (!m || !p || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    dnas_flat* f = new dnas_flat{dnas::FlatModel::build(m->machine, dnas::MutatorParams::fromC(*p))};
    f->flat.bind();
    *out = f;
    return DNAS_OK;
  });
}

const dnas_flat_model* dnas_flat_view(const dnas_flat* f) { return f ? &f->flat.view : nullptr; }
void dnas_flat_free(dnas_flat* f) { delete f; }

int dnas_fastseqs_read(const char* path, dnas_fastseqs** out) {
  if (!path || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    *out = new dnas_fastseqs{dnas::readFastSeqs(path)};
    return DNAS_OK;
  });
}
int64_t dnas_fastseqs_count(const dnas_fastseqs* f) { return f ? (int64_t)f->seqs.size() : 0; }
const char* dnas_fastseqs_name(const dnas_fastseqs* f, int64_t i) { return f->seqs[(size_t)i].name.c_str(); }
const char* dnas_fastseqs_seq(const dnas_fastseqs* f, int64_t i) { return f->seqs[(size_t)i].seq.c_str(); }
void dnas_fastseqs_free(dnas_fastseqs* f) { delete f; }

int dnas_stockholm_read(const char* path, dnas_pairs** out) {
  if (!path || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  return guarded([&] {
    dnas_pairs* p = new dnas_pairs{dnas::readStockholmPairs(path), {}};
    const dnas::AlignmentPairs& d = p->db;
    p->view = dnas_pairs_view{d.n, d.inSeqs.data(), d.inOff.data(), d.outSeqs.data(), d.outOff.data(),
                              d.cmIn.data(), d.cmInOff.data(), d.cmOut.data(), d.cmOutOff.data()};
    *out = p;
    return DNAS_OK;
  });
}
const dnas_pairs_view* dnas_pairs_get(const dnas_pairs* p) { return p ? &p->view : nullptr; }
void dnas_pairs_free(dnas_pairs* p) { delete p; }

// ---- pair alignment, host side (the GPU call is in pair_align_kernels.hip) ----------------------------------------------

int dnas_mutator_scores(const dnas_mutator_params* params, double* out) {
  if (!params || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    const dnas::MutatorParams p = dnas::MutatorParams::fromC(*params);
    // the same expressions FlatModel::build evaluates (PairScores::from holds 13 lengths; this entry takes all 32)
    dnas::MutatorParams head = p;
    if (head.pLen.size() > (size_t)dnas::kAlignMaxLen) head.pLen.resize(dnas::kAlignMaxLen);
    const dnas::PairScores s = dnas::PairScores::from(head);
    out[0] = s.delOpen; out[1] = s.tanDup; out[2] = s.noGap; out[3] = s.delExtend; out[4] = s.delEnd;
    for (int i = 0; i < 16; ++i) out[5 + i] = s.sub[i];
    for (size_t k = 0; k < p.pLen.size(); ++k) out[21 + k] = std::log(p.pLen[k]);
    return DNAS_OK;
  });
}

int dnas_align_pairs_host(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                          const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, uint8_t* out_ops,
                          const uint64_t* ops_off, uint32_t* out_n_ops, double* out_score, uint8_t* out_status) {
  if (const int rc = dnas::checkAlignArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_ops, ops_off, out_n_ops,
                                          out_score, out_status))
    return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    std::vector<uint8_t> ops;
    for (int64_t i = 0; i < n_pairs; ++i) {
      const int64_t I = in_off[i + 1] - in_off[i], O = out_off[i + 1] - out_off[i];
      out_score[i] = dnas::alignPairHost(sc, in_seqs + in_off[i], I, out_seqs + out_off[i], O, band, &ops);
      const bool path = out_score[i] > -std::numeric_limits<double>::infinity();
      out_status[i] = path ? DNAS_ALIGN_OK : DNAS_ALIGN_NO_PATH;
      out_n_ops[i] = path ? (uint32_t)ops.size() : 0;
      if (path) std::copy(ops.begin(), ops.end(), out_ops + ops_off[i]);
    }
    return DNAS_OK;
  });
}

int dnas_pair_likelihoods_host(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                               const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                               int exact_lse, double* out_ll) {
  if (const int rc = dnas::checkForwardArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_ll)) return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    for (int64_t i = 0; i < n_pairs; ++i)
      out_ll[i] = dnas::forwardPairHost(sc, in_seqs + in_off[i], in_off[i + 1] - in_off[i], out_seqs + out_off[i],
                                        out_off[i + 1] - out_off[i], band, out_rev != nullptr && out_rev[i] != 0, exact_lse != 0);
    return DNAS_OK;
  });
}

int dnas_pair_counts_host(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                          const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                          int exact_lse, double* out_counts, double* out_ll, double* out_pair_counts, double* out_pair_ll,
                          double* out_pair_ll_backward, uint8_t* out_status) {
  if (const int rc = dnas::checkCountsArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_counts, out_ll, out_pair_ll,
                                           out_status))
    return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    dnas::pairCountsHostAll(sc, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_rev, exact_lse != 0, out_counts, out_ll,
                            out_pair_counts, out_pair_ll, out_pair_ll_backward, out_status);
    return DNAS_OK;
  });
}

int dnas_pair_profiles_host(const dnas_mutator_params* params, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                            const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                            int exact_lse, int32_t anchor, int64_t n_positions, double* out_profile, int64_t* out_coverage,
                            double* out_pair_profiles, double* out_pair_ll, uint8_t* out_status) {
  if (const int rc = dnas::checkProfileArgs(params, band, n_pairs, in_seqs, in_off, out_seqs, out_off, anchor, n_positions, out_profile,
                                            out_coverage, out_pair_ll, out_status))
    return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    dnas::ProfileSum sum(params->n_len, anchor, n_positions, out_profile, out_coverage);
    dnas::pairProfilesHostAll(sc, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_rev, exact_lse != 0, &sum, out_pair_profiles,
                              out_pair_ll, out_status);
    return DNAS_OK;
  });
}

int dnas_baum_welch_pairs_host(const dnas_mutator_params* init, int32_t band, int64_t n_pairs, const int8_t* in_seqs,
                               const int64_t* in_off, const int8_t* out_seqs, const int64_t* out_off, const uint8_t* out_rev,
                               int exact_lse, int32_t max_iterations, dnas_mutator_params* out, int32_t* out_iterations,
                               dnas_mutator_params* out_trace_params, double* out_trace_ll, int32_t* out_n_trace) {
  if (!out) return dnas::fail(DNAS_E_INVALID, "pair counts: null argument");
  if (max_iterations < 0) return dnas::fail(DNAS_E_INVALID, "baum-welch on pairs: negative max_iterations");
  std::vector<double> pairLl((size_t)std::max<int64_t>(n_pairs, 1));
  std::vector<uint8_t> status((size_t)std::max<int64_t>(n_pairs, 1));
  double counts0[21 + 32], ll0 = 0;
  if (const int rc = dnas::checkCountsArgs(init, band, n_pairs, in_seqs, in_off, out_seqs, out_off, counts0, &ll0, pairLl.data(),
                                           status.data()))
    return rc;
  return guarded([&] {
    int32_t seenN = 0;
    const int rc = dnas::baumWelchLoop(
        *init, max_iterations,
        [&](const dnas_mutator_params& cur, double* counts, double* ll) {
          const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(cur));
          dnas::pairCountsHostAll(sc, band, n_pairs, in_seqs, in_off, out_seqs, out_off, out_rev, exact_lse != 0, counts, ll, nullptr,
                                  pairLl.data(), nullptr, status.data());
          return DNAS_OK;
        },
        [&](const dnas_mutator_params& cur, double ll) {
          if (out_trace_params) out_trace_params[seenN] = cur;
          if (out_trace_ll) out_trace_ll[seenN] = ll;
          ++seenN;
        },
        out, out_iterations);
    if (out_n_trace) *out_n_trace = seenN;
    return rc;
  });
}

int dnas_assign_reads_host(const dnas_mutator_params* params, int32_t band, int64_t n_originals, const int8_t* orig_seqs,
                           const int64_t* orig_off, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int strand_mode,
                           const int64_t* cand_off, const int64_t* cand_idx, int64_t* out_original, uint8_t* out_strand,
                           double* out_score, double* out_second, uint8_t* out_status, double* out_item_scores) {
  if (const int rc = dnas::checkAssignOriginals(params, band, n_originals, orig_seqs, orig_off)) return rc;
  if (const int rc = dnas::checkAssignReads(n_originals, n_reads, read_seqs, read_off, strand_mode, cand_off, cand_idx, out_original,
                                            out_strand, out_score, out_second, out_status))
    return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    dnas::assignReadsHost(sc, band, n_originals, orig_seqs, orig_off, n_reads, read_seqs, read_off, strand_mode, cand_off, cand_idx,
                          out_original, out_strand, out_score, out_second, out_status, out_item_scores);
    return DNAS_OK;
  });
}

int dnas_consensus_score_host_ex(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand,
                                 const int8_t* cand_seqs, const int64_t* cand_off, const int64_t* cluster_cand_off, int64_t n_reads,
                                 const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                                 const int64_t* cluster_read_off, int score_mode, int64_t* out_winner, double* out_total,
                                 double* out_second, uint8_t* out_status, double* out_totals, double* out_posterior) {
  if (const int rc = dnas::checkConsensusArgs(params, band, n_clusters, n_cand, cand_seqs, cand_off, cluster_cand_off, n_reads, read_seqs,
                                              read_off, read_strand, cluster_read_off, out_winner, out_total, out_second, out_status))
    return rc;
  if (const int rc = dnas::checkScoreMode(score_mode, out_posterior)) return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    std::vector<double> own;                               // the posteriors need every total
    if (out_posterior && !out_totals) {
      own.resize((size_t)n_cand + 1);
      out_totals = own.data();
    }
    dnas::consensusScoreHost(sc, band, n_clusters, cand_seqs, cand_off, cluster_cand_off, read_seqs, read_off, read_strand,
                             cluster_read_off, out_winner, out_total, out_second, out_status, out_totals, score_mode);
    if (out_posterior) dnas::consensusPosteriors(n_clusters, cluster_cand_off, out_status, out_totals, out_posterior);
    return DNAS_OK;
  });
}

int dnas_consensus_score_host(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, int64_t n_cand, const int8_t* cand_seqs,
                              const int64_t* cand_off, const int64_t* cluster_cand_off, int64_t n_reads, const int8_t* read_seqs,
                              const int64_t* read_off, const uint8_t* read_strand, const int64_t* cluster_read_off, int64_t* out_winner,
                              double* out_total, double* out_second, uint8_t* out_status, double* out_totals) {
  return dnas_consensus_score_host_ex(params, band, n_clusters, n_cand, cand_seqs, cand_off, cluster_cand_off, n_reads, read_seqs, read_off,
                                      read_strand, cluster_read_off, DNAS_SCORE_VITERBI, out_winner, out_total, out_second, out_status,
                                      out_totals, nullptr);
}

int dnas_cluster_reads_gated_host(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                                  double min_score_per_nt, int32_t max_edit_permille, int64_t n_reads, const int8_t* read_seqs,
                                  const int64_t* read_off, int64_t* out_root, int64_t* out_cluster, uint8_t* out_strand,
                                  uint8_t* out_status, int64_t** out_edge_ij, double** out_edge_score, uint8_t** out_edge_strand,
                                  int64_t* out_n_edges, dnas_cluster_stats* out_stats, dnas_cluster_gate_stats* out_gate) {
  if (out_stats) *out_stats = dnas_cluster_stats{};
  if (out_gate) *out_gate = dnas_cluster_gate_stats{};
  if (const int rc = dnas::checkClusterArgs(params, band, k, m, min_shared, n_reads, read_seqs, read_off, out_root, out_cluster, out_strand,
                                            out_status))
    return rc;
  if (const int rc = dnas::checkClusterGate(max_edit_permille)) return rc;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    std::vector<dnas::ClusterEdge> edges;
    dnas_cluster_stats stats;
    dnas::clusterReadsHost(sc, band, k, m, min_shared, min_score_per_nt, max_edit_permille, n_reads, read_seqs, read_off, out_root,
                           out_cluster, out_strand, out_status, &edges, nullptr, &stats, out_gate);
    if (out_stats) *out_stats = stats;
    return dnas::clusterExportEdges(edges, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges);
  });
}

int dnas_cluster_reads_host(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                            double min_score_per_nt, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, int64_t* out_root,
                            int64_t* out_cluster, uint8_t* out_strand, uint8_t* out_status, int64_t** out_edge_ij, double** out_edge_score,
                            uint8_t** out_edge_strand, int64_t* out_n_edges, dnas_cluster_stats* out_stats) {
  return dnas_cluster_reads_gated_host(params, band, k, m, min_shared, min_score_per_nt, -1, n_reads, read_seqs, read_off, out_root,
                                       out_cluster, out_strand, out_status, out_edge_ij, out_edge_score, out_edge_strand, out_n_edges,
                                       out_stats, nullptr);
}

int dnas_edit_distances_host(int64_t n_pairs, const int64_t* pair_ij, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                             int32_t* out_dist) {
  if (const int rc = dnas::checkEditArgs(n_pairs, pair_ij, n_reads, read_seqs, read_off, out_dist)) return rc;
  return guarded([&] {
    for (int64_t q = 0; q < n_pairs; ++q) {
      const int64_t i = pair_ij[2 * q], j = pair_ij[2 * q + 1];
      const int8_t *a = read_seqs + read_off[i], *b = read_seqs + read_off[j];
      const int64_t la = read_off[i + 1] - read_off[i], lb = read_off[j + 1] - read_off[j];
      out_dist[2 * q] = dnas::editDistanceHost(a, la, b, lb, false);
      out_dist[2 * q + 1] = dnas::editDistanceHost(a, la, b, lb, true);
    }
    return (int)DNAS_OK;
  });
}

int dnas_trim_reads_host(int64_t n_pairs, const int8_t* primer_seqs, const int64_t* primer_off, int64_t n_reads, const int8_t* read_seqs,
                         const int64_t* read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors, int32_t min_payload,
                         int32_t* out_pair, uint8_t* out_strand, int32_t* out_begin, int32_t* out_end, int32_t* out_edits,
                         int32_t* out_second, uint8_t* out_status) {
  if (const int rc = dnas::checkTrimArgs(n_pairs, primer_seqs, primer_off, n_reads, read_seqs, read_off, max_offset, max_edit_permille,
                                         anchors, min_payload, out_pair, out_strand, out_begin, out_end, out_edits, out_second, out_status))
    return rc;
  return guarded([&] {
    dnas::trimReadsHost(n_pairs, primer_seqs, primer_off, 0, n_reads, read_seqs, read_off, max_offset, max_edit_permille, anchors,
                        min_payload, out_pair, out_strand, out_begin, out_end, out_edits, out_second, out_status);
    return (int)DNAS_OK;
  });
}

int dnas_simulate_reads_host(const dnas_mutator_params* params, int64_t n_strands, const int8_t* strand_seqs, const int64_t* strand_off,
                             int64_t n_reads, const int64_t* read_strand, uint64_t seed, uint64_t first_index, double reverse_prob,
                             int want_ops, int8_t** out_seqs, int64_t** out_off, uint8_t** out_reversed, uint8_t** out_ops,
                             int64_t** out_ops_off, uint8_t* out_status) {
  if (const int rc = dnas::checkSimulateArgs(params, n_strands, strand_seqs, strand_off, n_reads, read_strand, reverse_prob, want_ops, out_seqs,
                                             out_off, out_reversed, out_ops, out_ops_off, out_status))
    return rc;
  return guarded([&] {
    const dnas::SimThresholds th = dnas::SimThresholds::from(*params, reverse_prob);
    std::vector<int8_t> seqs;
    std::vector<uint8_t> ops, reversed((size_t)n_reads);
    std::vector<int64_t> off(1, 0), opsOff(1, 0);
    for (int64_t r = 0; r < n_reads; ++r) {
      const int64_t s = read_strand[r];
      reversed[(size_t)r] = dnas::simulateReadHost(th, seed, first_index + (uint64_t)r, strand_seqs + strand_off[s],
                                                   strand_off[s + 1] - strand_off[s], &seqs, want_ops ? &ops : nullptr);
      off.push_back((int64_t)seqs.size());
      opsOff.push_back((int64_t)ops.size());
      out_status[r] = DNAS_SIM_OK;
    }
    return dnas::simulateHandOut(n_reads, seqs, off, reversed, want_ops, ops, opsOff, out_seqs, out_off, out_reversed, out_ops, out_ops_off);
  });
}

uint64_t dnas_simulate_draw_bits(uint64_t seed, uint64_t read, uint32_t position, uint32_t j) {
  return dnas::SimDraws(seed, read, position).bits(j);
}

int dnas_cluster_sketch_host(int32_t k, int32_t m, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, uint32_t* out_sig) {
  const dnas_mutator_params none{};
  std::vector<int64_t> i64((size_t)std::max<int64_t>(n_reads, 1));
  std::vector<uint8_t> u8((size_t)std::max<int64_t>(n_reads, 1));
  if (const int rc = dnas::checkClusterArgs(&none, 0, k, m, 0, n_reads, read_seqs, read_off, i64.data(), i64.data(), u8.data(), u8.data()))
    return rc;
  if (n_reads && !out_sig) return dnas::fail(DNAS_E_INVALID, "cluster reads: null argument");
  for (int64_t i = 0; i < n_reads; ++i)
    dnas::clusterSketchHost(read_seqs + read_off[i], read_off[i + 1] - read_off[i], k, m, out_sig + (size_t)i * (size_t)m);
  return DNAS_OK;
}

int dnas_cluster_candidates_host(const dnas_mutator_params* params, int32_t band, int32_t k, int32_t m, int32_t min_shared, int64_t n_reads,
                                 const int8_t* read_seqs, const int64_t* read_off, int64_t** out_cand_ij, double** out_cand_scores,
                                 int64_t* out_n_cand) {
  if (!out_cand_ij || !out_cand_scores || !out_n_cand) return dnas::fail(DNAS_E_INVALID, "cluster reads: null argument");
  *out_cand_ij = nullptr;
  *out_cand_scores = nullptr;
  *out_n_cand = 0;
  const size_t n1 = (size_t)std::max<int64_t>(n_reads, 1);
  return guarded([&] {
    std::vector<int64_t> root(n1), cluster(n1);
    std::vector<uint8_t> strand(n1), status(n1);
    if (const int rc = dnas::checkClusterArgs(params, band, k, m, min_shared, n_reads, read_seqs, read_off, root.data(), cluster.data(),
                                              strand.data(), status.data()))
      return rc;
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    std::vector<dnas::ClusterEdge> edges;
    std::vector<dnas::ClusterCandidate> cands;
    dnas_cluster_stats stats;
    dnas::clusterReadsHost(sc, band, k, m, min_shared, 0.0, -1, n_reads, read_seqs, read_off, root.data(), cluster.data(), strand.data(),
                           status.data(), &edges, &cands, &stats, nullptr);
    int64_t* ij = (int64_t*)malloc(std::max<size_t>(cands.size(), 1) * 2 * sizeof(int64_t));
    double* scores = (double*)malloc(std::max<size_t>(cands.size(), 1) * 2 * sizeof(double));
    if (!ij || !scores) {
      free(ij); free(scores);
      return dnas::fail(DNAS_E_NOMEM, "out of memory");
    }
    for (size_t c = 0; c < cands.size(); ++c) {
      ij[2 * c] = cands[c].i; ij[2 * c + 1] = cands[c].j;
      scores[2 * c] = cands[c].score[0]; scores[2 * c + 1] = cands[c].score[1];
    }
    *out_cand_ij = ij;
    *out_cand_scores = scores;
    *out_n_cand = (int64_t)cands.size();
    return (int)DNAS_OK;
  });
}

int dnas_cluster_consensus_host(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, const int8_t* tmpl_seqs,
                                const int64_t* tmpl_off, int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off,
                                const uint8_t* read_strand, const int64_t* cluster_read_off, int32_t rounds_max, int8_t** out_seqs,
                                int64_t* out_off, int32_t* out_rounds, uint8_t* out_converged, int32_t* out_voters, uint8_t* out_status) {
  if (const int rc = dnas::checkPolishArgs(params, band, n_clusters, tmpl_seqs, tmpl_off, n_reads, read_seqs, read_off, read_strand,
                                           cluster_read_off, rounds_max, out_seqs, out_off, out_rounds, out_converged, out_voters, out_status))
    return rc;
  *out_seqs = nullptr;
  return guarded([&] {
    const dnas::PairScores sc = dnas::PairScores::from(dnas::MutatorParams::fromC(*params));
    std::vector<std::vector<int8_t>> seqs;
    dnas::clusterConsensusHost(sc, band, n_clusters, tmpl_seqs, tmpl_off, read_seqs, read_off, read_strand, cluster_read_off, rounds_max,
                               &seqs, out_rounds, out_converged, out_voters, out_status);
    return dnas::polishExport(seqs, out_seqs, out_off);
  });
}

// Clusters of reads -> one message each (include/dnastore_amd.h): decode every read, make each cluster's candidate strands from
// its reads' messages, and let dnas_consensus_score pick.  A client of the C ABI like any other: what it adds is the candidates.
// polish_rounds > 0 (dnas_viterbi_clusters_ex): every cluster also gets a consensus read, whose message is one more candidate.
// score_mode and out_confidence (may be null) are dnas_viterbi_clusters_scored's; the other entries pass DNAS_SCORE_VITERBI and null.
static int viterbiClusters(dnas_model* model, const dnas_machine* machine, const dnas_mutator_params* params, int32_t band,
                           int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases, const int64_t* cluster_read_off,
                           int64_t n_clusters, int strand_mode, int32_t polish_rounds, char* out_sym, const uint64_t* out_offsets,
                           uint32_t* out_len, double* out_loglike, uint8_t* out_status, uint8_t* out_strand, int64_t* out_read,
                           double* out_total, double* out_second, int32_t* out_n_candidates, int32_t* out_votes,
                           uint8_t* out_cluster_status, uint8_t* out_source, int8_t** out_cons_seqs, int64_t* out_cons_off,
                           char* out_cons_sym, const uint64_t* cons_sym_offsets, uint32_t* out_cons_len, double* out_cons_loglike,
                           uint8_t* out_cons_status, int score_mode, double* out_confidence, dnas_consensus_stats* out_stats) {
  if (out_stats) *out_stats = dnas_consensus_stats{};
  if (polish_rounds < 0) return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_clusters: polish_rounds must be at least 0");
  if (polish_rounds > 0 && (!out_cons_seqs || !out_cons_off || !cons_sym_offsets || (n_clusters && (!out_source || !out_cons_sym || !out_cons_len || !out_cons_loglike || !out_cons_status))))
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_clusters: null argument");
  if (out_cons_seqs) *out_cons_seqs = nullptr;
  if (!model || !machine || !params || n_reads < 0 || n_clusters < 0 || !cluster_read_off)
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_clusters: bad argument");
  if (n_clusters && (!out_read || !out_total || !out_second || !out_n_candidates || !out_votes || !out_cluster_status))
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_clusters: null argument");
  if (n_reads && !out_strand) return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_clusters: null argument");
  if (cluster_read_off[0] != 0) return dnas::fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t c = 0; c < n_clusters; ++c)
    if (cluster_read_off[c + 1] < cluster_read_off[c]) return dnas::fail(DNAS_E_INVALID, "cluster " + std::to_string(c) + ": inconsistent read offsets");
  if (cluster_read_off[n_clusters] != n_reads)
    return dnas::fail(DNAS_E_INVALID, "dnas_viterbi_clusters: the clusters' read offsets end at " + std::to_string(cluster_read_off[n_clusters]) + ", not at " + std::to_string(n_reads));
  using clock = std::chrono::steady_clock;
  auto ms = [](clock::time_point a, clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const clock::time_point t0 = clock::now();
  if (const int rc = dnas_viterbi_batch_strands(model, n_reads, read_offsets, bases, strand_mode, out_sym, out_offsets, out_len, out_loglike,
                                                out_status, out_strand))
    return rc;
  const clock::time_point t1 = clock::now();
  return guarded([&] {
    std::vector<int8_t> cands, reads;
    std::vector<int64_t> candOff(1, 0), clCandOff(1, 0), readOff(1, 0), proposer;
    std::vector<int32_t> votes;
    int64_t encodeFailures = 0;
    static const char kBases[] = "ACGT";
    for (int64_t i = 0; i < n_reads; ++i) {
      for (uint64_t j = read_offsets[i]; j < read_offsets[i + 1]; ++j) reads.push_back((int8_t)bases[j]);
      readOff.push_back((int64_t)reads.size());
    }
    reads.push_back(0);                                  // (never a null pointer)
    // the consensus reads: every cluster's first read, in the orientation it was decoded in, polished by all of them, then decoded
    double polishMs = 0;
    if (polish_rounds > 0) {
      const clock::time_point p0 = clock::now();
      std::vector<int8_t> tmpl;
      std::vector<int64_t> tmplOff(1, 0);
      for (int64_t c = 0; c < n_clusters; ++c) {
        if (cluster_read_off[c + 1] > cluster_read_off[c]) {
          const int64_t i = cluster_read_off[c], O = readOff[(size_t)i + 1] - readOff[(size_t)i];
          const int8_t* const b = reads.data() + readOff[(size_t)i];
          for (int64_t j = 0; j < O; ++j) tmpl.push_back(out_strand[i] ? (int8_t)(3 - b[O - 1 - j]) : b[j]);
        }
        tmplOff.push_back((int64_t)tmpl.size());
      }
      tmpl.push_back(0);
      std::vector<int32_t> rounds((size_t)n_clusters + 1), voters((size_t)n_clusters + 1);
      std::vector<uint8_t> converged((size_t)n_clusters + 1), status((size_t)n_clusters + 1);
      if (const int rc = dnas_cluster_consensus(params, band, n_clusters, tmpl.data(), tmplOff.data(), n_reads, reads.data(), readOff.data(),
                                                out_strand, cluster_read_off, polish_rounds, dnas_model_device(model), 0, out_cons_seqs,
                                                out_cons_off, rounds.data(), converged.data(), voters.data(), status.data(), nullptr))
        return rc;
      std::vector<uint64_t> consOff((size_t)n_clusters + 1);
      for (int64_t c = 0; c <= n_clusters; ++c) consOff[(size_t)c] = (uint64_t)out_cons_off[c];
      if (const int rc = dnas_viterbi_batch(model, n_clusters, consOff.data(), (const uint8_t*)*out_cons_seqs, out_cons_sym, cons_sym_offsets,
                                            out_cons_len, out_cons_loglike, out_cons_status)) {
        dnas_free(*out_cons_seqs);
        *out_cons_seqs = nullptr;
        return rc;
      }
      polishMs = ms(p0, clock::now());
    } else if (out_cons_off) {
      for (int64_t c = 0; c <= n_clusters; ++c) out_cons_off[c] = 0;
    }
    const clock::time_point t1b = clock::now();
    // the candidates: per cluster the distinct strands its reads' messages encode to, in order of first appearance, then the
    // consensus read's if it is a new one (its proposer is -1)
    for (int64_t c = 0; c < n_clusters; ++c) {
      std::map<std::string, size_t> seen;                // strand -> its candidate
      for (int64_t i = cluster_read_off[c]; i < cluster_read_off[c + 1]; ++i) {
        if (out_status[i] != DNAS_READ_OK || out_len[i] == 0) continue;
        char* dna = nullptr;
        size_t nDna = 0;
        const int erc = dnas_encode_symbols(machine, out_sym + out_offsets[i], out_len[i], &dna, &nDna);
        if (erc == DNAS_E_NOMEM) throw std::bad_alloc();
        if (erc != DNAS_OK) {                            // not a message of this machine: no candidate
          ++encodeFailures;
          continue;
        }
        const std::string strand(dna, nDna);
        dnas_free(dna);
        const auto at = seen.find(strand);
        if (at != seen.end()) {
          ++votes[at->second];
          continue;
        }
        seen.emplace(strand, votes.size());
        for (char ch : strand) {
          const char* p = strchr(kBases, ch);
          if (!p || !ch) throw std::runtime_error(std::string("Unknown symbol ") + ch + " in an encoded strand");
          cands.push_back((int8_t)(p - kBases));
        }
        candOff.push_back((int64_t)cands.size());
        proposer.push_back(i);
        votes.push_back(1);
      }
      if (polish_rounds > 0 && out_cons_status[c] == DNAS_READ_OK && out_cons_len[c] != 0) {
        char* dna = nullptr;
        size_t nDna = 0;
        const int erc = dnas_encode_symbols(machine, out_cons_sym + cons_sym_offsets[c], out_cons_len[c], &dna, &nDna);
        if (erc == DNAS_E_NOMEM) throw std::bad_alloc();
        if (erc != DNAS_OK) {
          ++encodeFailures;
        } else {
          const std::string strand(dna, nDna);
          dnas_free(dna);
          if (seen.find(strand) == seen.end()) {
            for (char ch : strand) {
              const char* p = strchr(kBases, ch);
              if (!p || !ch) throw std::runtime_error(std::string("Unknown symbol ") + ch + " in an encoded strand");
              cands.push_back((int8_t)(p - kBases));
            }
            candOff.push_back((int64_t)cands.size());
            proposer.push_back(-1);
            votes.push_back(0);
          }
        }
      }
      clCandOff.push_back((int64_t)votes.size());
    }
    cands.push_back(0);                                  // (never a null pointer)
    const clock::time_point t2 = clock::now();
    const int64_t nCand = (int64_t)votes.size();
    std::vector<int64_t> winner((size_t)n_clusters + 1);
    dnas_consensus_stats st{};
    std::vector<double> posterior(out_confidence ? (size_t)nCand + 1 : 0);
    const int rc = dnas_consensus_score_ex(params, band, n_clusters, nCand, cands.data(), candOff.data(), clCandOff.data(), n_reads,
                                           reads.data(), readOff.data(), out_strand, cluster_read_off, dnas_model_device(model), score_mode,
                                           winner.data(), out_total, out_second, out_cluster_status, nullptr,
                                           out_confidence ? posterior.data() : nullptr, &st);
    if (rc != DNAS_OK) {
      if (out_cons_seqs && *out_cons_seqs) {
        dnas_free(*out_cons_seqs);
        *out_cons_seqs = nullptr;
      }
      return rc;
    }
    for (int64_t c = 0; c < n_clusters; ++c) {
      const int64_t w = winner[(size_t)c];
      out_read[c] = w < 0 ? -1 : proposer[(size_t)w];
      out_votes[c] = w < 0 ? 0 : votes[(size_t)w];
      out_n_candidates[c] = (int32_t)(clCandOff[(size_t)c + 1] - clCandOff[(size_t)c]);
      if (out_source) out_source[c] = w >= 0 && proposer[(size_t)w] < 0 ? 1 : 0;
      if (out_confidence) out_confidence[c] = w < 0 ? 0.0 : posterior[(size_t)w];
    }
    st.candidates = nCand;
    st.encode_failures = encodeFailures;
    st.decode_wall_ms = ms(t0, t1);
    st.candidates_wall_ms = ms(t1b, t2);
    st.rescore_wall_ms = ms(t2, clock::now());
    st.polish_wall_ms = polishMs;
    if (out_stats) *out_stats = st;
    return DNAS_OK;
  });
}

int dnas_viterbi_clusters_ex(dnas_model* model, const dnas_machine* machine, const dnas_mutator_params* params, int32_t band,
                             int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases, const int64_t* cluster_read_off,
                             int64_t n_clusters, int strand_mode, int32_t polish_rounds, char* out_sym, const uint64_t* out_offsets,
                             uint32_t* out_len, double* out_loglike, uint8_t* out_status, uint8_t* out_strand, int64_t* out_read,
                             double* out_total, double* out_second, int32_t* out_n_candidates, int32_t* out_votes,
                             uint8_t* out_cluster_status, uint8_t* out_source, int8_t** out_cons_seqs, int64_t* out_cons_off,
                             char* out_cons_sym, const uint64_t* cons_sym_offsets, uint32_t* out_cons_len, double* out_cons_loglike,
                             uint8_t* out_cons_status, dnas_consensus_stats* out_stats) {
  return viterbiClusters(model, machine, params, band, n_reads, read_offsets, bases, cluster_read_off, n_clusters, strand_mode, polish_rounds,
                         out_sym, out_offsets, out_len, out_loglike, out_status, out_strand, out_read, out_total, out_second,
                         out_n_candidates, out_votes, out_cluster_status, out_source, out_cons_seqs, out_cons_off, out_cons_sym,
                         cons_sym_offsets, out_cons_len, out_cons_loglike, out_cons_status, DNAS_SCORE_VITERBI, nullptr, out_stats);
}

int dnas_viterbi_clusters_scored(dnas_model* model, const dnas_machine* machine, const dnas_mutator_params* params, int32_t band,
                                 int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases, const int64_t* cluster_read_off,
                                 int64_t n_clusters, int strand_mode, int32_t polish_rounds, char* out_sym, const uint64_t* out_offsets,
                                 uint32_t* out_len, double* out_loglike, uint8_t* out_status, uint8_t* out_strand, int64_t* out_read,
                                 double* out_total, double* out_second, int32_t* out_n_candidates, int32_t* out_votes,
                                 uint8_t* out_cluster_status, uint8_t* out_source, int8_t** out_cons_seqs, int64_t* out_cons_off,
                                 char* out_cons_sym, const uint64_t* cons_sym_offsets, uint32_t* out_cons_len, double* out_cons_loglike,
                                 uint8_t* out_cons_status, int score_mode, double* out_confidence, dnas_consensus_stats* out_stats) {
  if (out_stats) *out_stats = dnas_consensus_stats{};
  if (out_cons_seqs) *out_cons_seqs = nullptr;
  if (const int rc = dnas::checkScoreMode(score_mode, out_confidence)) return rc;
  return viterbiClusters(model, machine, params, band, n_reads, read_offsets, bases, cluster_read_off, n_clusters, strand_mode, polish_rounds,
                         out_sym, out_offsets, out_len, out_loglike, out_status, out_strand, out_read, out_total, out_second,
                         out_n_candidates, out_votes, out_cluster_status, out_source, out_cons_seqs, out_cons_off, out_cons_sym,
                         cons_sym_offsets, out_cons_len, out_cons_loglike, out_cons_status, score_mode, out_confidence, out_stats);
}

int dnas_viterbi_clusters(dnas_model* model, const dnas_machine* machine, const dnas_mutator_params* params, int32_t band,
                          int64_t n_reads, const uint64_t* read_offsets, const uint8_t* bases, const int64_t* cluster_read_off,
                          int64_t n_clusters, int strand_mode, char* out_sym, const uint64_t* out_offsets, uint32_t* out_len,
                          double* out_loglike, uint8_t* out_status, uint8_t* out_strand, int64_t* out_read, double* out_total,
                          double* out_second, int32_t* out_n_candidates, int32_t* out_votes, uint8_t* out_cluster_status,
                          dnas_consensus_stats* out_stats) {
  return dnas_viterbi_clusters_ex(model, machine, params, band, n_reads, read_offsets, bases, cluster_read_off, n_clusters, strand_mode, 0,
                                  out_sym, out_offsets, out_len, out_loglike, out_status, out_strand, out_read, out_total, out_second,
                                  out_n_candidates, out_votes, out_cluster_status, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                  nullptr, nullptr, out_stats);
}

int dnas_alignment_expand(int32_t n_len, const int8_t* in, int64_t in_len, const int8_t* out, int64_t out_len, const uint8_t* ops,
                          int64_t n_ops, char* row_in, char* row_out, int32_t* cm_in, int32_t* cm_out, double* counts) {
  if (n_len < 0 || n_len > 32 || in_len < 0 || out_len < 0 || n_ops < 0 || (!in && in_len) || (!out && out_len) || (!ops && n_ops))
    return dnas::fail(DNAS_E_INVALID, "dnas_alignment_expand: bad argument");
  for (int64_t j = 0; j < in_len; ++j) if (in[j] < 0 || in[j] > 3) return dnas::fail(DNAS_E_BAD_BASE, "bad base");
  for (int64_t j = 0; j < out_len; ++j) if (out[j] < 0 || out[j] > 3) return dnas::fail(DNAS_E_BAD_BASE, "bad base");
  try {
    std::string r1, r2;
    dnas::expandAlignment(n_len, in, in_len, out, out_len, ops, n_ops, &r1, &r2, cm_in, cm_out, counts);
    if (row_in) memcpy(row_in, r1.c_str(), r1.size() + 1);
    if (row_out) memcpy(row_out, r2.c_str(), r2.size() + 1);
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

int dnas_stockholm_write(int64_t n_pairs, const char* const* names_in, const char* const* names_out, const char* const* rows_in,
                         const char* const* rows_out, char** text, size_t* len) {
  if (n_pairs < 0 || !text || !len || (n_pairs && (!names_in || !names_out || !rows_in || !rows_out)))
    return dnas::fail(DNAS_E_INVALID, "dnas_stockholm_write: bad argument");
  *text = nullptr;
  *len = 0;
  for (int64_t i = 0; i < n_pairs; ++i)
    if (!names_in[i] || !names_out[i] || !rows_in[i] || !rows_out[i]) return dnas::fail(DNAS_E_INVALID, "dnas_stockholm_write: null string");
  try {
    const std::string s = dnas::writeStockholm(n_pairs, names_in, names_out, rows_in, rows_out);
    char* buf = (char*)malloc(s.size() + 1);
    if (!buf) throw std::bad_alloc();
    memcpy(buf, s.c_str(), s.size() + 1);
    *text = buf;
    *len = s.size();
    return DNAS_OK;
  } catch (const std::bad_alloc&) {
    return dnas::fail(DNAS_E_NOMEM, "out of memory");
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_INVALID, e.what());
  }
}

// MutatorParams::writeJSON / MutatorCounts::writeJSON (mutator.cpp:6-16,108-124): the text the
// reference prints for --fit-error / --error-counts, default 6-digit ostream formatting.
int dnas_mutator_params_json(const dnas_mutator_params* p, char* buf, size_t cap) {
  if (!p || !buf || !cap) return dnas::fail(DNAS_E_INVALID, "null argument");
  return guarded([&] {
    const std::string s = dnas::MutatorParams::fromC(*p).toJSON();
    if (s.size() + 1 > cap) return dnas::fail(DNAS_E_INVALID, "buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1);
    return DNAS_OK;
  });
}
int dnas_mutator_counts_json(const double* counts, int32_t n_len, char* buf, size_t cap) {
  if (!counts || !buf || !cap || n_len < 0) return dnas::fail(DNAS_E_INVALID, "bad argument");
  return guarded([&] {
    auto trans = [](int i, int j) { return i != j && (i & 1) == (j & 1); };
    double nm = 0, ni = 0, nv = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) {
        const double c = counts[5 + i * 4 + j];
        if (i == j) nm += c; else if (trans(i, j)) ni += c; else nv += c;
      }
    // nMatch / nTransition / nTransversion are summed in the reference's loop order (mutator.cpp:180-196)
    nm = 0; for (int i = 0; i < 4; ++i) nm += counts[5 + i * 5];
    ni = 0; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) if (trans(i, j)) ni += counts[5 + i * 4 + j];
    nv = 0; for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) if (i != j && !trans(i, j)) nv += counts[5 + i * 4 + j];
    std::ostringstream o;
    o << "{\n";
    o << " \"nDelOpen\": " << counts[0] << ",\n";
    o << " \"nTanDup\": " << counts[1] << ",\n";
    o << " \"nNoGap\": " << counts[2] << ",\n";
    o << " \"nDelExtend\": " << counts[3] << ",\n";
    o << " \"nDelEnd\": " << counts[4] << ",\n";
    o << " \"nLen\": [ ";
    for (int k = 0; k < n_len; ++k) o << (k ? ", " : "") << counts[21 + k];
    o << " ],\n \"nSub\": [ ";
    for (int i = 0; i < 4; ++i) {
      o << (i ? ", " : "") << "[";
      for (int j = 0; j < 4; ++j) o << (j ? "," : "") << counts[5 + i * 4 + j];
      o << "]";
    }
    o << " ],\n";
    o << " \"nMatch\": " << nm << ",\n";
    o << " \"nTransition\": " << ni << ",\n";
    o << " \"nTransversion\": " << nv << "\n";
    o << "}\n";
    const std::string s = o.str();
    if (s.size() + 1 > cap) return dnas::fail(DNAS_E_INVALID, "buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1);
    return DNAS_OK;
  });
}

// decodeFastSeqs (viterbi.cpp:306-320): read the FASTA, build the input model once, decode every read on the GPU,
// keep names, drop comments.  device_id >= 0: that GPU.  device_id = -1: every GPU of the node -- the reads are dealt
// over the devices by length in snake order (longest first: 0..n-1, n-1..0, ...; what shard.partition does for the
// one-process-per-GPU bench), one host thread and one model per device, results back in file order.  The loop the
// reference runs serially (viterbi.cpp:312-318) has no dependence between reads, so nothing is exchanged.
// strands null: dnas_viterbi_batch, as ever; else dnas_viterbi_batch_strands in strand_mode, the strand of every read kept.
static int decode_shard(const dnas_flat_model* fm, int device, const std::vector<dnas::FastSeq>& reads, const std::vector<int64_t>& mine,
                        bool events, std::vector<std::string>* seqs, std::vector<double>* lls, std::vector<std::vector<uint64_t>>* evs,
                        std::string* tier, int strand_mode = DNAS_STRAND_FORWARD, std::vector<uint8_t>* strands = nullptr) {
  std::unique_ptr<dnas_model, void (*)(dnas_model*)> owner(nullptr, dnas_model_destroy);   // (destroying leaves dnas_last_error as it is)
  try {
    if (mine.empty()) return DNAS_OK;
    std::vector<std::vector<uint8_t>> toks;
    for (int64_t i : mine) toks.push_back(dnas::tokenizeDNA(reads[(size_t)i].seq, reads[(size_t)i].name));
    dnas_model* model = nullptr;
    int rc = dnas_model_create(fm, device, 0, &model);
    if (rc != DNAS_OK) return rc;
    owner.reset(model);
    *tier = dnas_model_tier(model);
    if (events && (rc = dnas_model_set_event_log(model, 1)) != DNAS_OK) return rc;
    // The slots are this function's own, 4 L + 64 symbols a read: a guess (a walk decodes a symbol per state it passes, however
    // short the read).  A read that overflows its slot has left there the length it needs (dnas_slot_needed), and the reads that
    // did are decoded once more, alone, in slots of that size.  A shard without one is the one call it ever was.
    std::vector<size_t> todo(mine.size()), cap(mine.size());
    for (size_t k = 0; k < mine.size(); ++k) { todo[k] = k; cap[k] = 4 * toks[k].size() + 64; }
    for (int pass = 0; !todo.empty(); ++pass) {
      std::vector<uint64_t> off{0}, outOff{0};
      std::vector<uint8_t> bases;
      for (size_t k : todo) {
        bases.insert(bases.end(), toks[k].begin(), toks[k].end());
        off.push_back(bases.size());
        outOff.push_back(outOff.back() + cap[k]);
      }
      const int64_t n = (int64_t)todo.size();
      std::vector<char> sym(outOff.back());
      std::vector<uint32_t> len((size_t)n);
      std::vector<double> ll((size_t)n);
      std::vector<uint8_t> st((size_t)n);
      if (bases.empty()) bases.push_back(0);
      std::vector<uint8_t> strand((size_t)n, 0);
      if (strands)
        rc = dnas_viterbi_batch_strands(model, n, off.data(), bases.data(), strand_mode, sym.data(), outOff.data(), len.data(), ll.data(), st.data(), strand.data());
      else
        rc = dnas_viterbi_batch(model, n, off.data(), bases.data(), sym.data(), outOff.data(), len.data(), ll.data(), st.data());
      if (rc != DNAS_OK) return rc;
      std::vector<size_t> again;
      for (int64_t j = 0; j < n; ++j) {
        const size_t k = todo[(size_t)j], at = (size_t)mine[k];
        if (st[(size_t)j] == DNAS_READ_TRACEBACK_FAIL) return dnas::fail(DNAS_E_DEVICE, "Traceback failure");
        if (st[(size_t)j] == DNAS_READ_OUT_OVERFLOW) {
          const uint64_t need = dnas_slot_needed(sym.data() + outOff[(size_t)j], cap[k]);
          if (pass > 0 || need <= cap[k]) return dnas::fail(DNAS_E_DEVICE, "decoded string overflowed its slot");
          cap[k] = (size_t)need;
          again.push_back(k);
          continue;
        }
        if (strands) (*strands)[at] = strand[(size_t)j];
        (*seqs)[at].assign(sym.data() + outOff[(size_t)j], len[(size_t)j]);
        (*lls)[at] = ll[(size_t)j];
        if (events) {               // (of this call: the next one drops its log)
          int64_t ne = 0;
          rc = dnas_model_read_events(model, j, nullptr, 0, &ne);
          if (rc != DNAS_OK) return rc;
          std::vector<uint64_t>& e = (*evs)[at];
          e.resize((size_t)ne);
          if (ne && (rc = dnas_model_read_events(model, j, e.data(), ne, &ne)) != DNAS_OK) return rc;
        }
      }
      todo.swap(again);
    }
    return DNAS_OK;
  } catch (const std::exception& e) {
    return dnas::fail(DNAS_E_DEVICE, e.what());
  }
}

int dnas_decode_fastseqs(const char* fasta_path, const dnas_machine* m, const dnas_mutator_params* p, int device_id,
                         dnas_decoded** out) {
  return dnas_decode_fastseqs_ex(fasta_path, m, p, device_id, 0, out);
}

// strand_mode < 0: dnas_decode_fastseqs_ex (dnas_viterbi_batch per device)
static int decode_fastseqs_any(const char* fasta_path, const dnas_machine* m, const dnas_mutator_params* p, int device_id,
                               int want_events, int strand_mode, dnas_decoded** out) {
  if (!fasta_path || !m || !p || !out) return dnas::fail(DNAS_E_INVALID, "null argument");
  *out = nullptr;
  dnas_flat* flat = nullptr;
  int rc = guarded([&] {
    const std::vector<dnas::FastSeq> reads = dnas::readFastSeqs(fasta_path);
    int r = dnas_flatten(m, p, &flat);
    if (r != DNAS_OK) return r;
    const int64_t n = (int64_t)reads.size();
    std::vector<int> devices = dnas::pickDevices(device_id);
    if (devices.empty()) return dnas::fail(DNAS_E_DEVICE, "no HIP device available");
    if ((int64_t)devices.size() > std::max<int64_t>(n, 1)) devices.resize((size_t)std::max<int64_t>(n, 1));   // no device without reads
    // deal the reads: by length, longest first, in snake order
    std::vector<int64_t> len((size_t)n);
    for (int64_t i = 0; i < n; ++i) len[(size_t)i] = (int64_t)reads[(size_t)i].seq.size();
    const size_t W = devices.size();
    const std::vector<std::vector<int64_t>> shard = dnas::snakeDeal(len, W);
    std::unique_ptr<dnas_decoded> d(new dnas_decoded());
    std::vector<std::string> seqs((size_t)n);
    std::vector<double> lls((size_t)n, 0.);
    d->events.resize((size_t)n);
    std::vector<std::string> tiers(W);
    d->strand.assign((size_t)n, 0);
    std::vector<uint8_t>* const strands = strand_mode >= 0 ? &d->strand : nullptr;
    r = dnas::forEachDevice(devices, [&](size_t w) {
      return decode_shard(dnas_flat_view(flat), devices[w], reads, shard[w], want_events != 0, &seqs, &lls, &d->events, &tiers[w], strand_mode, strands);
    });
    if (r != DNAS_OK) return r;
    for (int64_t i = 0; i < n; ++i) {
      dnas::FastSeq fs;
      fs.name = reads[(size_t)i].name;  // viterbi.cpp:315: name kept, comment dropped
      fs.seq = std::move(seqs[(size_t)i]);
      d->seqs.push_back(std::move(fs));
      d->loglike.push_back(lls[(size_t)i]);
    }
    for (const auto& t : tiers) if (!t.empty()) { d->tier = t; break; }
    d->devices = (int)W;
    *out = d.release();
    return DNAS_OK;
  });
  if (flat) dnas_flat_free(flat);
  return rc;
}

int dnas_decode_fastseqs_ex(const char* fasta_path, const dnas_machine* m, const dnas_mutator_params* p, int device_id,
                            int want_events, dnas_decoded** out) {
  return decode_fastseqs_any(fasta_path, m, p, device_id, want_events, -1, out);
}

int dnas_decode_fastseqs_strands(const char* fasta_path, const dnas_machine* m, const dnas_mutator_params* p, int device_id,
                                 int want_events, int strand_mode, dnas_decoded** out) {
  if (strand_mode < DNAS_STRAND_FORWARD || strand_mode > DNAS_STRAND_BOTH)
    return dnas::fail(DNAS_E_INVALID, "dnas_decode_fastseqs_strands: strand_mode must be DNAS_STRAND_FORWARD, _REVERSE or _BOTH");
  return decode_fastseqs_any(fasta_path, m, p, device_id, want_events, strand_mode, out);
}

// What a read that overflowed its slot left there (viterbi_kernels.hip, store_needed_len).
uint64_t dnas_slot_needed(const char* slot, uint64_t cap) {
  if (!slot || cap < 8) return 0;
  uint64_t n = 0;
  for (int k = 0; k < 8; ++k) n |= (uint64_t)(uint8_t)slot[k] << (8 * k);
  return n;
}

int dnas_decoded_strand(const dnas_decoded* d, int64_t i) { return d && i >= 0 && (size_t)i < d->strand.size() ? d->strand[(size_t)i] : 0; }

// out[i] = 3 - bases[n - 1 - i]: the other strand of a read, base codes 0..3 = ACGT.
int dnas_reverse_complement(const uint8_t* bases, size_t n, uint8_t* out) {
  if ((!bases || !out) && n) return dnas::fail(DNAS_E_INVALID, "dnas_reverse_complement: null argument");
  for (size_t i = 0; i < n; ++i) {
    const uint8_t b = bases[n - 1 - i];
    if (b > 3) return dnas::fail(DNAS_E_BAD_BASE, "base code > 3 at offset " + std::to_string(n - 1 - i));
    out[i] = (uint8_t)(3 - b);
  }
  return DNAS_OK;
}

int64_t dnas_decoded_count(const dnas_decoded* d) { return d ? (int64_t)d->seqs.size() : 0; }
const char* dnas_decoded_name(const dnas_decoded* d, int64_t i) { return d->seqs[(size_t)i].name.c_str(); }
const char* dnas_decoded_seq(const dnas_decoded* d, int64_t i) { return d->seqs[(size_t)i].seq.c_str(); }
double dnas_decoded_loglike(const dnas_decoded* d, int64_t i) { return d->loglike[(size_t)i]; }
const char* dnas_decoded_tier(const dnas_decoded* d) { return d ? d->tier.c_str() : ""; }
int dnas_decoded_devices(const dnas_decoded* d) { return d ? d->devices : 0; }
int64_t dnas_decoded_events(const dnas_decoded* d, int64_t i, const uint64_t** events) {
  if (!d || i < 0 || (size_t)i >= d->events.size()) return 0;
  if (events) *events = d->events[(size_t)i].data();
  return (int64_t)d->events[(size_t)i].size();
}
void dnas_decoded_free(dnas_decoded* d) { delete d; }

}  // extern "C"
