#include "polish.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

#include "../errors.hpp"

namespace dnas {

namespace {

int checkSeqs(const char* what, int64_t n, const int8_t* seqs, const int64_t* off) {
  if (n == 0) return DNAS_OK;
  if (!seqs || !off) return fail(DNAS_E_INVALID, "cluster consensus: null argument");
  if (off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t i = 0; i < n; ++i) {
    const int64_t len = off[i + 1] - off[i];
    if (len < 0) return fail(DNAS_E_INVALID, std::string(what) + " " + std::to_string(i) + ": inconsistent offsets");
    if (len > kAlignMaxSeq) return fail(DNAS_E_UNSUPPORTED, std::string(what) + " " + std::to_string(i) + ": longer than " + std::to_string(kAlignMaxSeq));
  }
  for (int64_t j = 0; j < off[n]; ++j) if (seqs[j] < 0 || seqs[j] > 3) return fail(DNAS_E_BAD_BASE, "bad base");
  return DNAS_OK;
}

}  // namespace

int checkPolishArgs(const dnas_mutator_params* params, int32_t band, int64_t n_clusters, const int8_t* tmpl_seqs, const int64_t* tmpl_off,
                    int64_t n_reads, const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand,
                    const int64_t* cluster_read_off, int32_t rounds_max, int8_t* const* out_seqs, const int64_t* out_off,
                    const int32_t* out_rounds, const uint8_t* out_converged, const int32_t* out_voters, const uint8_t* out_status) {
  if (!params || n_clusters < 0 || n_reads < 0) return fail(DNAS_E_INVALID, "cluster consensus: bad argument");
  if (band < DNAS_ALIGN_FULL) return fail(DNAS_E_INVALID, "cluster consensus: band must be DNAS_ALIGN_FULL (-1) or at least 0");
  if (rounds_max < 0) return fail(DNAS_E_INVALID, "cluster consensus: rounds_max must be at least 0");
  if (params->n_len < 0) return fail(DNAS_E_INVALID, "negative pLen length");
  if (params->n_len > kAlignMaxLen) return fail(DNAS_E_UNSUPPORTED, "cluster consensus: more than 13 duplication lengths");
  if (!out_seqs || !out_off) return fail(DNAS_E_INVALID, "cluster consensus: null argument");
  if (n_clusters && (!out_rounds || !out_converged || !out_voters || !out_status)) return fail(DNAS_E_INVALID, "cluster consensus: null argument");
  if (!cluster_read_off) return fail(DNAS_E_INVALID, "cluster consensus: null argument");
  if (cluster_read_off[0] != 0) return fail(DNAS_E_INVALID, "offset arrays must start at 0");
  for (int64_t c = 0; c < n_clusters; ++c)
    if (cluster_read_off[c + 1] < cluster_read_off[c]) return fail(DNAS_E_INVALID, "cluster " + std::to_string(c) + ": inconsistent read offsets");
  if (cluster_read_off[n_clusters] != n_reads)
    return fail(DNAS_E_INVALID, "cluster consensus: the clusters' read offsets end at " + std::to_string(cluster_read_off[n_clusters]) + ", not at " + std::to_string(n_reads));
  if (int rc = checkSeqs("template", n_clusters, tmpl_seqs, tmpl_off)) return rc;
  if (int rc = checkSeqs("read", n_reads, read_seqs, read_off)) return rc;
  if (read_strand)
    for (int64_t i = 0; i < n_reads; ++i)
      if (read_strand[i] > 1) return fail(DNAS_E_INVALID, "read " + std::to_string(i) + ": strand must be 0 or 1");
  return DNAS_OK;
}

int32_t polishRoundHost(const PairScores& sc, int64_t band, const std::vector<int8_t>& t, const std::vector<std::vector<int8_t>>& reads,
                        std::vector<int8_t>* out) {
  const int64_t I = (int64_t)t.size();
  std::vector<uint32_t> tab(polishWords(I), 0);
  std::vector<uint8_t> ops;
  for (const std::vector<int8_t>& b : reads) {
    const double score = alignPairHost(sc, t.data(), I, b.data(), (int64_t)b.size(), band, &ops);
    if (!(score > -std::numeric_limits<double>::infinity())) continue;
    ++tab[0];
    int64_t ip = 0, op = 0;
    for (size_t c = 0; c < ops.size();) {
      const unsigned kind = ops[c] & 3u;
      if (kind == kOpMatch) {
        ++tab[polishM(ip, b[(size_t)op])];
        ++ip; ++op; ++c;
      } else if (kind == kOpDelete) {
        ++tab[polishD(ip)];
        ++ip; ++c;
      } else {
        int64_t L = 0;
        while (c < ops.size() && (ops[c] & 3u) == kOpDup) { ++L; ++c; }
        for (int64_t k = 0; k < std::min<int64_t>(L, DNAS_POLISH_MAX_INSERT); ++k) {
          ++tab[polishN(ip, (int)k)];
          ++tab[polishB(ip, (int)k, b[(size_t)(op + k)])];
        }
        op += L;
      }
    }
  }
  out->clear();
  for (int64_t g = 0; g <= I; ++g) {
    const PolishGap e = polishEmitGap(tab.data(), g, I, t.data());
    for (int j = 0; j < e.n; ++j) out->push_back((int8_t)((e.bases >> (2 * j)) & 3u));
  }
  return (int32_t)tab[0];
}

void clusterConsensusHost(const PairScores& sc, int64_t band, int64_t n_clusters, const int8_t* tmpl_seqs, const int64_t* tmpl_off,
                          const int8_t* read_seqs, const int64_t* read_off, const uint8_t* read_strand, const int64_t* cluster_read_off,
                          int32_t rounds_max, std::vector<std::vector<int8_t>>* seqs, int32_t* out_rounds, uint8_t* out_converged,
                          int32_t* out_voters, uint8_t* out_status) {
  seqs->assign((size_t)n_clusters, {});
  std::vector<std::vector<int8_t>> oriented;
  std::vector<int8_t> next;
  for (int64_t c = 0; c < n_clusters; ++c) {
    std::vector<int8_t>& t = (*seqs)[(size_t)c];
    t.assign(tmpl_seqs + tmpl_off[c], tmpl_seqs + tmpl_off[c + 1]);
    const int64_t r0 = cluster_read_off[c], r1 = cluster_read_off[c + 1];
    oriented.assign((size_t)(r1 - r0), {});
    for (int64_t i = r0; i < r1; ++i) {
      const int8_t* const b = read_seqs + read_off[i];
      const int64_t O = read_off[i + 1] - read_off[i];
      std::vector<int8_t>& o = oriented[(size_t)(i - r0)];
      o.resize((size_t)O);
      for (int64_t j = 0; j < O; ++j) o[(size_t)j] = read_strand && read_strand[i] ? (int8_t)(3 - b[O - 1 - j]) : b[j];
    }
    PolishCluster st;
    if (r1 == r0) { st.status = DNAS_POLISH_NO_READS; st.active = false; }
    for (int32_t run = 1; st.active && run <= rounds_max; ++run) {
      const int32_t V = polishRoundHost(sc, band, t, oriented, &next);
      st.after(V, next != t, run, rounds_max);
      if (V) t.swap(next);
    }
    out_rounds[c] = st.rounds;
    out_converged[c] = st.converged;
    out_voters[c] = st.voters;
    out_status[c] = st.status;
  }
}

int polishExport(const std::vector<std::vector<int8_t>>& seqs, int8_t** out_seqs, int64_t* out_off) {
  size_t total = 0;
  for (const auto& s : seqs) total += s.size();
  int8_t* buf = (int8_t*)malloc(std::max<size_t>(total, 1));
  if (!buf) return fail(DNAS_E_NOMEM, "out of memory");
  out_off[0] = 0;
  for (size_t c = 0; c < seqs.size(); ++c) {
    if (!seqs[c].empty()) memcpy(buf + out_off[c], seqs[c].data(), seqs[c].size());
    out_off[c + 1] = out_off[c] + (int64_t)seqs[c].size();
  }
  *out_seqs = buf;
  return DNAS_OK;
}

}  // namespace dnas
