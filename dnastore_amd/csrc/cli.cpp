// dnastore -- command-line driver with the reference's flags and output formats
// (reference t/dnastore.cpp:34-251) for everything on and around the error-decoding path:
// --load-machine / --compose-machine / --save-machine, the exact --encode-* / --decode-* arms,
// -V/--decode-viterbi with the --error-* model (GPU), --error-counts and --fit-error (GPU), and --align-pairs (GPU), which
// makes the Stockholm database the last two read out of two FASTA files, and --assign-reads (GPU), which first finds out which
// read of a pool belongs to which original.  -V with --cluster-file decodes clusters of reads to one message each;
// --cluster-reads (GPU) forms the clusters of a pool without originals or labels, -V with --cluster-auto does both.
// --trim-reads (GPU) is the front of all of these: it finds each raw read's primer pair and cuts the payload out.
// --simulate-reads (GPU) makes a pool: reads of the originals sampled from the error model, with their true alignments on request.
// --outer-code n,k,L is the last stage: --outer-encode turns a file into the strands of a Reed-Solomon code across strands,
// --outer-decode on any -V run assembles the decoded messages into the file again (GPU).
// It is a client of the C ABI in include/dnastore_amd.h only.
//
// Not provided: the `-l k` de Bruijn code builder (reference src/builder.cpp; its output is
// platform dependent).  Without --load-machine, `-l 4 -c 4` resolves to the
// canonical machine data/l4c4.json when DNASTORE_L4C4 names it; other lengths are refused.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/dnastore_amd.h"

namespace {

struct Options {
  int length = 12, controls = 4, verbose = 2, device = 0, alignBand = 32, clusterKmer = 12, clusterSketch = 32, clusterMinShared = 2, clusterPolish = 0, clusterMaxEdit = -1;
  std::string loadMachine, saveMachine, encodeFile, decodeFile, encodeString, decodeString, encodeBits, decodeBits,
      decodeViterbi, errorFile, fitError, errorCounts, fitPairs, countPairs, profilePairs, profileAnchor = "start", alignPairs, alignReads, assignReads, assignOriginals, assignStrands = "forward", clusterFile, clusterReads, clusterScore = "viterbi";
  std::vector<std::string> clusterAdd;
  std::string trimReads, trimPrimers, trimAnchors = "both", trimSelect;
  int trimMaxOffset = 8, trimMaxEdit = 250, trimMinPayload = 0;
  bool trimOptionGiven = false;
  std::string simulateReads, simulateSeed = "0";
  int simulateCoverage = 1;
  double simulateReverse = 0;
  bool simulateShuffle = false, simulateStockholm = false, simulateOptionGiven = false;
  std::string outerCode, outerEncode, outerDecode;
  long long outerBlocks = -1;
  std::vector<std::string> compose;
  bool raw = false, errorGlobal = false, strictGuides = false, help = false, bothStrands = false, reverseStrand = false, assignStockholm = false, clusterTable = false, clusterAuto = false, clusterPolishGiven = false, clusterMaxEditGiven = false, clusterScoreGiven = false;
  double subProb = .01, ivRatio = 10, dupProb = .001, delOpen = .001, delExt = .01, assignMinMargin = 0, clusterMinScore = 0;
};

const char* kHelp =
    "Allowed options:\n"
    "  -h [ --help ]                 display this help message\n"
    "  -l [ --length ] arg (=12)     length of k-mers in de Bruijn graph (sets the error model's pLen to length/2)\n"
    "  -c [ --controls ] arg (=4)    number of control words\n"
    "  -L [ --load-machine ] arg     load machine from JSON file\n"
    "  -S [ --save-machine ] arg     save machine to JSON file\n"
    "  -C [ --compose-machine ] arg  load machine from JSON file and compose in front of primary machine\n"
    "  -e [ --encode-file ] arg      encode binary file to FASTA on stdout\n"
    "  -d [ --decode-file ] arg      decode FASTA file to binary on stdout\n"
    "  -E [ --encode-string ] arg    encode ASCII string to FASTA on stdout\n"
    "  -D [ --decode-string ] arg    decode DNA sequence to binary on stdout\n"
    "  -b [ --encode-bits ] arg      encode string of bits and control symbols to FASTA on stdout\n"
    "  -B [ --decode-bits ] arg      decode DNA sequence to string of bits and control symbols on stdout\n"
    "  -V [ --decode-viterbi ] arg   decode FASTA file using Viterbi algorithm (MI355X)\n"
    "  --both-strands                with -V: reads of unknown orientation -- decode each read and its reverse complement, keep the likelier\n"
    "  --reverse-strand              with -V: decode the reverse complement of every read (the second reads of a paired run)\n"
    "  --cluster-file arg            with -V: one cluster name per read, in the FASTA's order -- print one record per cluster (in order of\n"
    "                                first appearance): of the messages its reads decode to, the one whose strand explains all of\n"
    "                                the cluster's reads best under the error model (--align-band applies)\n"
    "  --cluster-table               with --cluster-file: tab-separated lines instead: name, reads, candidates, votes, total, margin, symbols\n"
    "  --cluster-polish arg (=0)     with -V and --cluster-file or --cluster-auto: polish every cluster's first read by all its reads for\n"
    "                                at most arg rounds and let the decode of that consensus read be one more candidate; --cluster-table\n"
    "                                then has one more column, source: 0 = a read's message, 1 = the consensus read's\n"
    "  --cluster-score arg (=viterbi) with -V and --cluster-file or --cluster-auto: viterbi compares a cluster's candidates by the score of\n"
    "                                each read's best alignment, forward by each read's likelihood summed over all alignments in the\n"
    "                                band; with forward, --cluster-table has one more last column, confidence: the winner's posterior\n"
    "                                among the cluster's candidates (0 without a winner)\n"
    "  --cluster-auto                with -V, instead of --cluster-file: form the clusters from the reads themselves, as --cluster-reads does\n"
    "  --cluster-reads arg           FASTA file of a pool of reads of either strand: print one cluster name per read, in the FASTA's order,\n"
    "                                as --cluster-file reads them -- reads are joined when their k-mer sketches share positions and the\n"
    "                                error model scores one as a copy of the other (--align-band applies) (MI355X)\n"
    "  --cluster-add arg             with --cluster-reads, repeatable: one more FASTA file of reads that joins the pool as a batch of its\n"
    "                                own, in command-line order -- the output is that of --cluster-reads on the files concatenated\n"
    "  --cluster-kmer arg (=12)      length of the k-mers of the sketch (1 .. 31)\n"
    "  --cluster-sketch arg (=32)    positions of the sketch: 16, 32 or 64\n"
    "  --cluster-min-shared arg (=2) sketch positions two reads must share to be scored; 0 = score every pair\n"
    "  --cluster-min-score arg (=0)  the score per base of the second read, in nats, from which two reads are joined\n"
    "  --cluster-max-edit arg (=-1)  with --cluster-reads or --cluster-auto: score only the pairs whose edit distance, in the better\n"
    "                                orientation, is at most arg thousandths of the longer read (0 .. 1000); -1 = score every pair\n"
    "  --trim-reads arg              FASTA file of a pool of raw reads: find the primer pair (--trim-primers) that frames each read, on either\n"
    "                                strand, and print the payloads between the primers, oriented forward, as FASTA: >name primer=<the\n"
    "                                forward primer's name> strand=+|- edits=<forward>,<reverse>; the counts per status go to stderr (MI355X;\n"
    "                                on a machine without a GPU the host statement runs)\n"
    "  --trim-primers arg            FASTA file of the primers F0, R0, F1, R1, ..., both of a pair as they appear on the forward strand\n"
    "  --trim-max-offset arg (=8)    bases of adapter or junk a primer may have outside it; -1 = search the whole read\n"
    "  --trim-max-edit arg (=250)    edits a primer may have, in thousandths of its length (0 .. 1000)\n"
    "  --trim-anchors arg (=both)    both | either: either keeps a read that has only one of its two primers\n"
    "  --trim-min-payload arg (=0)   bases that must remain between the primers\n"
    "  --trim-select arg             print only the reads of the pair whose forward primer has this name\n"
    "  --simulate-reads arg          FASTA file of original strands: sample reads of them from the error model (--error-*) and print them\n"
    "                                as FASTA, named <original>/<n>, a read handed out reverse-complemented with strand=- after its name\n"
    "                                (MI355X; on a machine without a GPU the host statement runs: the reads are the same)\n"
    "  --simulate-coverage arg (=1)  reads per original\n"
    "  --simulate-seed arg (=0)      the seed: it alone fixes the reads\n"
    "  --simulate-reverse arg (=0)   probability that a read is handed out as its reverse complement\n"
    "  --simulate-shuffle            permute the reads' order (Python's random.Random(seed).shuffle of the list of originals)\n"
    "  --simulate-stockholm          instead of the reads, print the Stockholm database of their true alignments, as --fit-error reads it\n"
    "  --outer-code arg              n,k,L: the outer code -- Reed-Solomon RS(n, k) over GF(2^8) across blocks of n strands whose records\n"
    "                                are 3 bytes of strand number, a CRC-8 and L body bytes\n"
    "  --outer-encode arg            binary file: print its strands as FASTA, named s<number>, each record through the machine's byte\n"
    "                                encoder (needs --outer-code; MI355X, on a machine without a GPU the host statement runs)\n"
    "  --outer-decode arg            with -V, per read or per cluster: instead of printing the messages, take them as records, correct\n"
    "                                lost and wrong strands, write the file to arg and print the report as JSON (needs --outer-code and\n"
    "                                --outer-blocks; records are weighted by the confidence under --cluster-score forward, else 1)\n"
    "  --outer-blocks arg            the blocks of the file, as --outer-encode reported them on stderr\n"
    "  -r [ --raw ]                  strip headers from FASTA output; just print raw sequence\n"
    "  --error-sub-prob arg (=0.01)  substitution probability for error model\n"
    "  --error-iv-ratio arg (=10)    transition/transversion ratio for error model\n"
    "  --error-dup-prob arg (=0.001) tandem duplication probability for error model\n"
    "  --error-del-open arg (=0.001) deletion opening probability for error model\n"
    "  --error-del-ext arg (=0.01)   deletion extension probability for error model\n"
    "  --error-global                force global alignment in error model (disallow partial reads)\n"
    "  -F [ --error-file ] arg       load error model from file\n"
    "  -f [ --fit-error ] arg        train error model on Stockholm database of pairwise alignments and print to stdout\n"
    "  --error-counts arg            estimate posterior expected counts of various different types of error from Stockholm database\n"
    "  --strict-guides               treat alignments in Stockholm database as strict truth, not just hints\n"
    "  --align-pairs arg             FASTA file of original strands: align each to its read (--align-reads) under the error model and\n"
    "                                print the Stockholm database of the alignments to stdout (MI355X); one original pairs with all reads\n"
    "  --align-reads arg             FASTA file of the reads, paired with the originals by order\n"
    "  --fit-pairs arg               FASTA file of original strands: train the error model on them and their reads (--align-reads)\n"
    "                                over every alignment inside the band, no guide alignment, and print it to stdout (MI355X)\n"
    "  --count-pairs arg             the posterior expected counts of the error types from the same two files (MI355X)\n"
    "  --profile-pairs arg           the same counts kept per position of the original, from the same two files: where along the\n"
    "                                strands the substitutions, deletions and duplications fell, as one JSON object (MI355X)\n"
    "  --profile-anchor arg (=start) start | end: the end of the original the positions count from\n"
    "  --align-band arg (=32)        diagonals either side of the pair's corner-to-corner band; -1 = the full matrix\n"
    "  --assign-reads arg            FASTA file of a pool of reads: find the original (--assign-originals) each came from under the error\n"
    "                                model and print one line per read: read, original or *, + or -, score, margin (MI355X)\n"
    "  --assign-originals arg        FASTA file of the library of original strands\n"
    "  --assign-strands arg (=forward)  forward | reverse | both: the orientations of every read that are tried\n"
    "  --assign-stockholm            instead of the lines, align every assigned read to its original and print the Stockholm database\n"
    "  --assign-min-margin arg (=0)  with --assign-stockholm: leave out reads whose margin over the runner-up original is smaller\n"
    "  -v [ --verbose ] arg (=2)     verbosity level\n"
    "  --device arg (=0)             GPU to use; -1 = every GPU of the node, reads (or alignment pairs) dealt over them\n";

[[noreturn]] void die(const std::string& msg) {
  std::cerr << msg << std::endl;
  exit(1);
}

void check(int rc) {
  if (rc != DNAS_OK) {
    // the reference prints e.what() and still exits 0 for the exceptions it catches in main
    // (dnastore.cpp:245-250: parse errors, cyclic machines, ...); missing files exit 1 (Fail, util.cpp:47-54).
    // Failures that are not reference exceptions -- no GPU, out of device memory, an unsupported or invalid
    // request -- must not look like success: an empty stdout with exit 0 would feed empty decodes downstream.
    std::cerr << dnas_last_error() << std::endl;
    const bool referenceException = rc == DNAS_E_PARSE || rc == DNAS_E_CYCLIC || rc == DNAS_E_NOT_DNA || rc == DNAS_E_BAD_BASE;
    exit(referenceException ? 0 : (rc == DNAS_E_IO ? 1 : 2));
  }
}

void writeFasta(std::ostream& out, const char* name, const std::string& seq, bool raw) {
  if (raw) { out << seq << "\n"; return; }
  out << ">" << name << "\n";
  for (size_t i = 0; i < seq.size(); i += 50) out << seq.substr(i, 50) << "\n";   // fastseq.h:14
}

Options parse(int argc, char** argv) {
  Options o;
  auto need = [&](int& i, const std::string& flag) -> std::string {
    if (i + 1 >= argc) die("the required argument for option '" + flag + "' is missing");
    return argv[++i];
  };
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i], val;
    bool hasVal = false;
    if (a.rfind("--", 0) == 0) {
      const size_t eq = a.find('=');
      if (eq != std::string::npos) { val = a.substr(eq + 1); a = a.substr(0, eq); hasVal = true; }
    } else if (a.size() > 2 && a[0] == '-' && a[1] != '-') {   // -l4, -v0
      val = a.substr(2); a = a.substr(0, 2); hasVal = true;
    }
    auto arg = [&]() { return hasVal ? val : need(i, a); };
    if (a == "-h" || a == "--help") o.help = true;
    else if (a == "-l" || a == "--length") o.length = atoi(arg().c_str());
    else if (a == "-c" || a == "--controls") o.controls = atoi(arg().c_str());
    else if (a == "-L" || a == "--load-machine") o.loadMachine = arg();
    else if (a == "-S" || a == "--save-machine") o.saveMachine = arg();
    else if (a == "-C" || a == "--compose-machine") o.compose.push_back(arg());
    else if (a == "-e" || a == "--encode-file") o.encodeFile = arg();
    else if (a == "-d" || a == "--decode-file") o.decodeFile = arg();
    else if (a == "-E" || a == "--encode-string") o.encodeString = arg();
    else if (a == "-D" || a == "--decode-string") o.decodeString = arg();
    else if (a == "-b" || a == "--encode-bits") o.encodeBits = arg();
    else if (a == "-B" || a == "--decode-bits") o.decodeBits = arg();
    else if (a == "-V" || a == "--decode-viterbi") o.decodeViterbi = arg();
    else if (a == "--both-strands") o.bothStrands = true;
    else if (a == "--reverse-strand") o.reverseStrand = true;
    else if (a == "--cluster-file") o.clusterFile = arg();
    else if (a == "--cluster-table") o.clusterTable = true;
    else if (a == "--cluster-auto") o.clusterAuto = true;
    else if (a == "--cluster-score") { o.clusterScore = arg(); o.clusterScoreGiven = true; }
    else if (a == "--cluster-polish") { o.clusterPolish = atoi(arg().c_str()); o.clusterPolishGiven = true; }
    else if (a == "--cluster-reads") o.clusterReads = arg();
    else if (a == "--cluster-add") o.clusterAdd.push_back(arg());
    else if (a == "--cluster-kmer") o.clusterKmer = atoi(arg().c_str());
    else if (a == "--cluster-sketch") o.clusterSketch = atoi(arg().c_str());
    else if (a == "--cluster-min-shared") o.clusterMinShared = atoi(arg().c_str());
    else if (a == "--cluster-min-score") o.clusterMinScore = atof(arg().c_str());
    else if (a == "--cluster-max-edit") { o.clusterMaxEdit = atoi(arg().c_str()); o.clusterMaxEditGiven = true; }
    else if (a == "--trim-reads") o.trimReads = arg();
    else if (a == "--trim-primers") o.trimPrimers = arg();
    else if (a == "--trim-max-offset") { o.trimMaxOffset = atoi(arg().c_str()); o.trimOptionGiven = true; }
    else if (a == "--trim-max-edit") { o.trimMaxEdit = atoi(arg().c_str()); o.trimOptionGiven = true; }
    else if (a == "--trim-anchors") { o.trimAnchors = arg(); o.trimOptionGiven = true; }
    else if (a == "--trim-min-payload") { o.trimMinPayload = atoi(arg().c_str()); o.trimOptionGiven = true; }
    else if (a == "--trim-select") { o.trimSelect = arg(); o.trimOptionGiven = true; }
    else if (a == "--simulate-reads") o.simulateReads = arg();
    else if (a == "--simulate-coverage") { o.simulateCoverage = atoi(arg().c_str()); o.simulateOptionGiven = true; }
    else if (a == "--simulate-seed") { o.simulateSeed = arg(); o.simulateOptionGiven = true; }
    else if (a == "--simulate-reverse") { o.simulateReverse = atof(arg().c_str()); o.simulateOptionGiven = true; }
    else if (a == "--simulate-shuffle") { o.simulateShuffle = true; o.simulateOptionGiven = true; }
    else if (a == "--simulate-stockholm") { o.simulateStockholm = true; o.simulateOptionGiven = true; }
    else if (a == "--outer-code") o.outerCode = arg();
    else if (a == "--outer-encode") o.outerEncode = arg();
    else if (a == "--outer-decode") o.outerDecode = arg();
    else if (a == "--outer-blocks") o.outerBlocks = atoll(arg().c_str());
    else if (a == "-r" || a == "--raw") o.raw = true;
    else if (a == "--error-sub-prob") o.subProb = atof(arg().c_str());
    else if (a == "--error-iv-ratio") o.ivRatio = atof(arg().c_str());
    else if (a == "--error-dup-prob") o.dupProb = atof(arg().c_str());
    else if (a == "--error-del-open") o.delOpen = atof(arg().c_str());
    else if (a == "--error-del-ext") o.delExt = atof(arg().c_str());
    else if (a == "--error-global") o.errorGlobal = true;
    else if (a == "-F" || a == "--error-file") o.errorFile = arg();
    else if (a == "-f" || a == "--fit-error") o.fitError = arg();
    else if (a == "--error-counts") o.errorCounts = arg();
    else if (a == "--strict-guides") o.strictGuides = true;
    else if (a == "--align-pairs") o.alignPairs = arg();
    else if (a == "--fit-pairs") o.fitPairs = arg();
    else if (a == "--count-pairs") o.countPairs = arg();
    else if (a == "--profile-pairs") o.profilePairs = arg();
    else if (a == "--profile-anchor") o.profileAnchor = arg();
    else if (a == "--align-reads") o.alignReads = arg();
    else if (a == "--align-band") o.alignBand = atoi(arg().c_str());
    else if (a == "--assign-reads") o.assignReads = arg();
    else if (a == "--assign-originals") o.assignOriginals = arg();
    else if (a == "--assign-strands") o.assignStrands = arg();
    else if (a == "--assign-stockholm") o.assignStockholm = true;
    else if (a == "--assign-min-margin") o.assignMinMargin = atof(arg().c_str());
    else if (a == "-v" || a == "--verbose") o.verbose = atoi(arg().c_str());
    else if (a == "--device") o.device = atoi(arg().c_str());
    else if (a == "--nocolor") {}
    else if (a == "--log") (void)arg();
    else die("unrecognised option '" + a + "'");
  }
  return o;
}

std::string slurp(const std::string& path, const char* what) {
  std::ifstream in(path, std::ios::binary);
  if (!in) die(std::string(what) + " not found");
  std::stringstream ss;
  ss << in.rdbuf();
  return ss.str();
}

void tokens(const char* name, const char* seq, std::vector<int8_t>& dst) {
  static const char kAlphabet[] = "ACGTacgt";
  for (const char* c = seq; *c; ++c) {
    const char* at = strchr(kAlphabet, *c);
    if (!at) die(std::string("Unknown symbol ") + *c + " in sequence " + name + " (alphabet is ACGT)");
    dst.push_back((int8_t)((at - kAlphabet) & 3));
  }
}

// dnas_align_pairs over pair i = (ins[inOff[i]..), outs[outOff[i]..)), then the Stockholm database of the alignments on stdout;
// a pair without one is named on stderr and left out.
void printAlignments(const Options& o, const dnas_mutator_params& mut, std::vector<int8_t>& ins, const std::vector<int64_t>& inOff,
                     std::vector<int8_t>& outs, const std::vector<int64_t>& outOff, const std::vector<const char*>& namesIn,
                     const std::vector<const char*>& namesOut) {
  const int64_t n = (int64_t)namesOut.size();
  ins.push_back(0); outs.push_back(0);                             // (never a null pointer)
  std::vector<uint64_t> opsOff(1, 0);
  for (int64_t i = 0; i < n; ++i) opsOff.push_back((uint64_t)(inOff[(size_t)i + 1] + outOff[(size_t)i + 1]));
  std::vector<uint8_t> ops((size_t)opsOff.back() + 1), status((size_t)n + 1);
  std::vector<uint32_t> nOps((size_t)n + 1);
  std::vector<double> score((size_t)n + 1);
  dnas_align_stats st;
  check(dnas_align_pairs(&mut, o.alignBand, n, ins.data(), inOff.data(), outs.data(), outOff.data(), o.device, 0, ops.data(), opsOff.data(),
                         nOps.data(), score.data(), status.data(), &st));
  if (o.verbose >= 3)
    std::cerr << "Pair alignment: " << st.cells << " cells in " << st.batches << " batches, fill " << st.fill_ms << " ms, traceback "
              << st.traceback_ms << " ms" << std::endl;
  std::vector<std::string> rowsIn, rowsOut;
  std::vector<const char*> nameIn, nameOut;
  for (int64_t i = 0; i < n; ++i) {
    const char* name = namesOut[(size_t)i];
    if (status[(size_t)i] != DNAS_ALIGN_OK || nOps[(size_t)i] == 0) {
      std::cerr << "No alignment for " << name << ": "
                << (status[(size_t)i] == DNAS_ALIGN_NO_PATH ? "the error model has no path between the two sequences"
                    : status[(size_t)i] == DNAS_ALIGN_TOO_LARGE ? "the pair is too large for the GPU's memory"
                    : status[(size_t)i] == DNAS_ALIGN_OK ? "both sequences are empty" : "traceback failed") << std::endl;
      continue;
    }
    std::string r1(nOps[(size_t)i] + 1, '\0'), r2(nOps[(size_t)i] + 1, '\0');
    check(dnas_alignment_expand(mut.n_len, ins.data() + inOff[(size_t)i], inOff[(size_t)i + 1] - inOff[(size_t)i], outs.data() + outOff[(size_t)i],
                                outOff[(size_t)i + 1] - outOff[(size_t)i], ops.data() + opsOff[(size_t)i], nOps[(size_t)i], &r1[0], &r2[0],
                                nullptr, nullptr, nullptr));
    r1.pop_back(); r2.pop_back();
    rowsIn.push_back(r1); rowsOut.push_back(r2);
    nameIn.push_back(namesIn[(size_t)i]);
    nameOut.push_back(name);
  }
  std::vector<const char*> pIn, pOut;
  for (size_t k = 0; k < rowsIn.size(); ++k) { pIn.push_back(rowsIn[k].c_str()); pOut.push_back(rowsOut[k].c_str()); }
  char* text = nullptr;
  size_t len = 0;
  check(dnas_stockholm_write((int64_t)rowsIn.size(), nameIn.data(), nameOut.data(), pIn.data(), pOut.data(), &text, &len));
  std::cout.write(text, (std::streamsize)len);
  dnas_free(text);
}

// dnas_cluster_reads over the reads of a FASTA file -> one cluster name per read, in file order.
std::vector<std::string> clusterNames(const Options& o, const dnas_mutator_params& mut, const dnas_fastseqs* fs) {
  if (o.alignBand < DNAS_ALIGN_FULL) die("--align-band must be -1 (the full matrix) or at least 0");
  if (o.clusterKmer < 1 || o.clusterKmer > 31) die("--cluster-kmer must be 1 .. 31");
  if (o.clusterSketch != 16 && o.clusterSketch != 32 && o.clusterSketch != 64) die("--cluster-sketch must be 16, 32 or 64");
  if (o.clusterMinShared < 0) die("--cluster-min-shared must be at least 0");
  if (o.clusterMaxEdit < -1 || o.clusterMaxEdit > 1000) die("--cluster-max-edit must be -1 .. 1000");
  const int64_t n = dnas_fastseqs_count(fs);
  std::vector<int8_t> reads;
  std::vector<int64_t> readOff(1, 0);
  for (int64_t i = 0; i < n; ++i) {
    tokens(dnas_fastseqs_name(fs, i), dnas_fastseqs_seq(fs, i), reads);
    readOff.push_back((int64_t)reads.size());
  }
  reads.push_back(0);                                              // (never a null pointer)
  std::vector<int64_t> root((size_t)n + 1), cluster((size_t)n + 1);
  std::vector<uint8_t> strand((size_t)n + 1), status((size_t)n + 1);
  dnas_cluster_stats st;
  dnas_cluster_gate_stats gate;
  check(dnas_cluster_reads_gated(&mut, o.alignBand, o.clusterKmer, o.clusterSketch, o.clusterMinShared, o.clusterMinScore, o.clusterMaxEdit,
                                 n, reads.data(), readOff.data(), o.device, root.data(), cluster.data(), strand.data(), status.data(),
                                 nullptr, nullptr, nullptr, nullptr, &st, &gate));
  if (o.verbose >= 3)
    std::cerr << "Read clustering: " << st.clusters << " clusters; " << st.candidates << " of " << st.pairs << " pairs scored, " << st.edges
              << " edges, " << st.strand_conflicts << " strand conflicts, " << st.cells << " cells in " << st.chunks << " chunks; sketch "
              << st.sketch_ms << " ms, filter " << st.filter_ms << " ms, score " << st.score_ms << " ms, fold " << st.fold_ms << " ms"
              << std::endl;
  if (o.verbose >= 3 && o.clusterMaxEdit >= 0)
    std::cerr << "Edit-distance gate: " << gate.passed << " of " << gate.tested << " candidates passed, " << gate.long_pairs
              << " on the long route, " << gate.word_steps << " word steps; gate " << gate.gate_ms << " ms" << std::endl;
  std::vector<std::string> names;
  for (int64_t i = 0; i < n; ++i) names.push_back("cluster" + std::to_string(cluster[(size_t)i]));
  return names;
}

// --trim-reads: dnas_trim_reads over the reads of a FASTA file and the primer pairs of another -> the payloads, oriented forward,
// as FASTA on stdout, the counts per status on stderr.
void trimPool(const Options& o) {
  if (o.trimMaxOffset < -1) die("--trim-max-offset must be -1 (the whole read) or at least 0");
  if (o.trimMaxEdit < 0 || o.trimMaxEdit > 1000) die("--trim-max-edit must be 0 .. 1000");
  if (o.trimAnchors != "both" && o.trimAnchors != "either") die("--trim-anchors must be both or either");
  if (o.trimMinPayload < 0) die("--trim-min-payload must be at least 0");
  dnas_fastseqs *fp = nullptr, *fr = nullptr;
  check(dnas_fastseqs_read(o.trimPrimers.c_str(), &fp));
  check(dnas_fastseqs_read(o.trimReads.c_str(), &fr));
  const int64_t np = dnas_fastseqs_count(fp), n = dnas_fastseqs_count(fr);
  if (np % 2) die(std::to_string(np) + " primers in " + o.trimPrimers + ": the records are F0, R0, F1, R1, ...");
  int64_t select = -1;
  for (int64_t k = 0; k < np / 2; ++k)
    if (!o.trimSelect.empty() && select < 0 && o.trimSelect == dnas_fastseqs_name(fp, 2 * k)) select = k;
  if (!o.trimSelect.empty() && select < 0) die("--trim-select: no forward primer is named " + o.trimSelect);
  std::vector<int8_t> primers, reads;
  std::vector<int64_t> primerOff(1, 0), readOff(1, 0);
  for (int64_t q = 0; q < np; ++q) {
    tokens(dnas_fastseqs_name(fp, q), dnas_fastseqs_seq(fp, q), primers);
    primerOff.push_back((int64_t)primers.size());
    const int64_t m = primerOff[(size_t)q + 1] - primerOff[(size_t)q];
    if (m < 1 || m > 64) die(std::string("primer ") + dnas_fastseqs_name(fp, q) + " must have 1 .. 64 bases");
  }
  for (int64_t i = 0; i < n; ++i) {
    tokens(dnas_fastseqs_name(fr, i), dnas_fastseqs_seq(fr, i), reads);
    readOff.push_back((int64_t)reads.size());
  }
  primers.push_back(0); reads.push_back(0);                          // (never a null pointer)
  std::vector<int32_t> pair((size_t)n + 1), begin((size_t)n + 1), end((size_t)n + 1), edits(2 * (size_t)n + 2), second((size_t)n + 1);
  std::vector<uint8_t> strand((size_t)n + 1), status((size_t)n + 1);
  const int anchors = o.trimAnchors == "either" ? DNAS_TRIM_EITHER : DNAS_TRIM_BOTH;
  if (dnas_has_device_code() && dnas_device_count() > 0) {
    dnas_trim_stats st;
    check(dnas_trim_reads(np / 2, primers.data(), primerOff.data(), n, reads.data(), readOff.data(), o.trimMaxOffset, o.trimMaxEdit, anchors,
                          o.trimMinPayload, o.device, pair.data(), strand.data(), begin.data(), end.data(), edits.data(), second.data(),
                          status.data(), &st));
    if (o.verbose >= 3)
      std::cerr << "Read trimming: " << st.items << " items in " << st.chunks << " pair chunks on " << st.devices << " devices, " << st.columns
                << " columns; kernels " << st.kernel_ms << " ms" << std::endl;
  } else {
    std::cerr << "No GPU: trimming with the host statement" << std::endl;
    check(dnas_trim_reads_host(np / 2, primers.data(), primerOff.data(), n, reads.data(), readOff.data(), o.trimMaxOffset, o.trimMaxEdit,
                               anchors, o.trimMinPayload, pair.data(), strand.data(), begin.data(), end.data(), edits.data(), second.data(),
                               status.data()));
  }
  int64_t counts[3] = {0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    ++counts[status[(size_t)i] < 3 ? status[(size_t)i] : 1];
    if (status[(size_t)i] != DNAS_TRIM_OK || (select >= 0 && pair[(size_t)i] != select)) continue;
    const int8_t* read = reads.data() + readOff[(size_t)i];
    std::string seq;
    if (strand[(size_t)i])
      for (int32_t c = end[(size_t)i] - 1; c >= begin[(size_t)i]; --c) seq += "ACGT"[3 - read[c]];
    else
      for (int32_t c = begin[(size_t)i]; c < end[(size_t)i]; ++c) seq += "ACGT"[read[c]];
    const std::string header = std::string(dnas_fastseqs_name(fr, i)) + " primer=" + dnas_fastseqs_name(fp, 2 * (int64_t)pair[(size_t)i]) +
                               " strand=" + (strand[(size_t)i] ? "-" : "+") + " edits=" + std::to_string(edits[2 * (size_t)i]) + "," +
                               std::to_string(edits[2 * (size_t)i + 1]);
    writeFasta(std::cout, header.c_str(), seq, o.raw);
  }
  std::cerr << "Trimmed reads: " << counts[DNAS_TRIM_OK] << " trimmed, " << counts[DNAS_TRIM_NO_ANCHOR] << " without primers, "
            << counts[DNAS_TRIM_TOO_SHORT] << " too short, of " << n << std::endl;
  dnas_fastseqs_free(fp);
  dnas_fastseqs_free(fr);
}

// Python's random.Random(seed).shuffle for a seed below 2^64: MT19937 seeded by init_by_array with the seed's 32-bit words (one
// word for a seed below 2^32), x[i] swapped with x[randbelow(i + 1)] for i = n - 1 .. 1, randbelow by rejection of the top bits.
class PythonRandom {
 public:
  explicit PythonRandom(uint64_t seed) {
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    const int len = key[1] ? 2 : 1;
    mt_[0] = 19650218u;
    for (int i = 1; i < 624; ++i) mt_[i] = 1812433253u * (mt_[i - 1] ^ (mt_[i - 1] >> 30)) + (uint32_t)i;
    int i = 1, j = 0;
    for (int k = 624; k; --k) {
      mt_[i] = (mt_[i] ^ ((mt_[i - 1] ^ (mt_[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
      if (++i >= 624) { mt_[0] = mt_[623]; i = 1; }
      if (++j >= len) j = 0;
    }
    for (int k = 623; k; --k) {
      mt_[i] = (mt_[i] ^ ((mt_[i - 1] ^ (mt_[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
      if (++i >= 624) { mt_[0] = mt_[623]; i = 1; }
    }
    mt_[0] = 0x80000000u;
  }
  uint32_t next() {
    if (at_ >= 624) {
      for (int k = 0; k < 624; ++k) {
        const uint32_t y = (mt_[k] & 0x80000000u) | (mt_[(k + 1) % 624] & 0x7FFFFFFFu);
        mt_[k] = mt_[(k + 397) % 624] ^ (y >> 1) ^ (y & 1u ? 0x9908B0DFu : 0u);
      }
      at_ = 0;
    }
    uint32_t y = mt_[at_++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9D2C5680u;
    y ^= (y << 15) & 0xEFC60000u;
    return y ^ (y >> 18);
  }
  uint32_t below(uint32_t n) {                             // n >= 1
    int bits = 0;
    while (bits < 32 && (n >> bits)) ++bits;
    for (;;) {
      const uint32_t r = next() >> (32 - bits);
      if (r < n) return r;
    }
  }
  template <class T>
  void shuffle(std::vector<T>& x) {
    for (size_t i = x.size(); i-- > 1;) std::swap(x[i], x[below((uint32_t)i + 1)]);
  }

 private:
  uint32_t mt_[624];
  int at_ = 624;
};

// --simulate-reads: dnas_simulate_reads over the strands of a FASTA file -> the reads as FASTA, or the Stockholm database of their
// true alignments, on stdout.
void simulatePool(const Options& o, const dnas_mutator_params& mut) {
  if (o.simulateCoverage < 1) die("--simulate-coverage must be at least 1");
  if (!(o.simulateReverse >= 0 && o.simulateReverse <= 1)) die("--simulate-reverse must be 0 .. 1");
  char* endp = nullptr;
  const uint64_t seed = strtoull(o.simulateSeed.c_str(), &endp, 10);
  if (o.simulateSeed.empty() || *endp || o.simulateSeed[0] == '-') die("--simulate-seed must be a number 0 .. 2^64 - 1");
  dnas_fastseqs* fs = nullptr;
  check(dnas_fastseqs_read(o.simulateReads.c_str(), &fs));
  const int64_t ns = dnas_fastseqs_count(fs);
  if (ns >= ((int64_t)1 << 31) / o.simulateCoverage) die("--simulate-reads: 2^31 reads or more");
  std::vector<int8_t> strands;
  std::vector<int64_t> strandOff(1, 0), readStrand;
  for (int64_t s = 0; s < ns; ++s) {
    tokens(dnas_fastseqs_name(fs, s), dnas_fastseqs_seq(fs, s), strands);
    strandOff.push_back((int64_t)strands.size());
    for (int c = 0; c < o.simulateCoverage; ++c) readStrand.push_back(s);
  }
  if (o.simulateShuffle) PythonRandom(seed).shuffle(readStrand);
  const int64_t n = (int64_t)readStrand.size();
  strands.push_back(0); readStrand.push_back(0);                     // (never a null pointer)
  int8_t* seqs = nullptr;
  int64_t *off = nullptr, *opsOff = nullptr;
  uint8_t *reversed = nullptr, *ops = nullptr;
  std::vector<uint8_t> status((size_t)n + 1);
  const int wantOps = o.simulateStockholm ? 1 : 0;
  if (dnas_has_device_code() && dnas_device_count() > 0) {
    dnas_simulate_stats st;
    check(dnas_simulate_reads(&mut, ns, strands.data(), strandOff.data(), n, readStrand.data(), seed, 0, o.simulateReverse, wantOps, o.device, 0,
                              &seqs, &off, &reversed, &ops, &opsOff, status.data(), &st));
    if (o.verbose >= 3)
      std::cerr << "Read simulation: " << st.bases_in << " bases in, " << st.bases_out << " out, " << st.ops << " ops in " << st.batches
                << " batches on " << st.devices << " devices; count " << st.count_ms << " ms, write " << st.write_ms << " ms" << std::endl;
  } else {
    std::cerr << "No GPU: simulating with the host statement" << std::endl;
    check(dnas_simulate_reads_host(&mut, ns, strands.data(), strandOff.data(), n, readStrand.data(), seed, 0, o.simulateReverse, wantOps, &seqs,
                                   &off, &reversed, &ops, &opsOff, status.data()));
  }
  std::vector<int64_t> made((size_t)ns + 1, 0);
  std::vector<std::string> names, rowsIn, rowsOut;
  std::vector<const char*> namesIn;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t s = readStrand[(size_t)i], len = off[i + 1] - off[i];
    const std::string name = std::string(dnas_fastseqs_name(fs, s)) + "/" + std::to_string(++made[(size_t)s]);
    if (status[(size_t)i] != DNAS_SIM_OK) {
      std::cerr << "No read " << name << ": it is too large for the GPU's memory" << std::endl;
      continue;
    }
    if (!o.simulateStockholm) {
      std::string seq;
      for (int64_t c = 0; c < len; ++c) seq += "ACGT"[seqs[off[i] + c] & 3];
      writeFasta(std::cout, (name + (reversed[i] ? " strand=-" : "")).c_str(), seq, o.raw);
      continue;
    }
    const int64_t nOps = opsOff[i + 1] - opsOff[i];
    if (nOps == 0) {
      std::cerr << "No alignment for " << name << ": both sequences are empty" << std::endl;
      continue;
    }
    std::vector<int8_t> fwd((size_t)len + 1);                        // the read before the reversal: what the ops describe
    for (int64_t c = 0; c < len; ++c) fwd[(size_t)c] = reversed[i] ? (int8_t)(3 - seqs[off[i] + len - 1 - c]) : seqs[off[i] + c];
    std::string r1((size_t)nOps + 1, '\0'), r2((size_t)nOps + 1, '\0');
    check(dnas_alignment_expand(mut.n_len, strands.data() + strandOff[(size_t)s], strandOff[(size_t)s + 1] - strandOff[(size_t)s], fwd.data(), len,
                                ops + opsOff[i], nOps, &r1[0], &r2[0], nullptr, nullptr, nullptr));
    r1.pop_back(); r2.pop_back();
    rowsIn.push_back(r1); rowsOut.push_back(r2);
    names.push_back(name);
    namesIn.push_back(dnas_fastseqs_name(fs, s));
  }
  if (o.simulateStockholm) {
    std::vector<const char*> pIn, pOut, pNames;
    for (size_t k = 0; k < rowsIn.size(); ++k) { pIn.push_back(rowsIn[k].c_str()); pOut.push_back(rowsOut[k].c_str()); pNames.push_back(names[k].c_str()); }
    char* text = nullptr;
    size_t len = 0;
    check(dnas_stockholm_write((int64_t)rowsIn.size(), namesIn.data(), pNames.data(), pIn.data(), pOut.data(), &text, &len));
    std::cout.write(text, (std::streamsize)len);
    dnas_free(text);
  }
  dnas_free(seqs); dnas_free(off); dnas_free(reversed); dnas_free(ops); dnas_free(opsOff);
  dnas_fastseqs_free(fs);
}

// The same over a pool that arrives file by file: the reads of --cluster-reads, then one batch per --cluster-add file, through
// a dnas_clusterer.
std::vector<std::string> clusterNamesBatched(const Options& o, const dnas_mutator_params& mut, const std::vector<std::string>& files) {
  if (o.alignBand < DNAS_ALIGN_FULL) die("--align-band must be -1 (the full matrix) or at least 0");
  if (o.clusterKmer < 1 || o.clusterKmer > 31) die("--cluster-kmer must be 1 .. 31");
  if (o.clusterSketch != 16 && o.clusterSketch != 32 && o.clusterSketch != 64) die("--cluster-sketch must be 16, 32 or 64");
  if (o.clusterMinShared < 0) die("--cluster-min-shared must be at least 0");
  if (o.clusterMaxEdit < -1 || o.clusterMaxEdit > 1000) die("--cluster-max-edit must be -1 .. 1000");
  if (o.device < 0) die("--cluster-add keeps the pool on one GPU: --device must name it");
  dnas_clusterer* h = nullptr;
  check(dnas_clusterer_create(&mut, o.alignBand, o.clusterKmer, o.clusterSketch, o.clusterMinShared, o.clusterMinScore, o.clusterMaxEdit,
                              o.device, &h));
  for (const std::string& file : files) {
    dnas_fastseqs* fs = nullptr;
    check(dnas_fastseqs_read(file.c_str(), &fs));
    const int64_t n = dnas_fastseqs_count(fs);
    std::vector<int8_t> reads;
    std::vector<int64_t> readOff(1, 0);
    for (int64_t i = 0; i < n; ++i) {
      tokens(dnas_fastseqs_name(fs, i), dnas_fastseqs_seq(fs, i), reads);
      readOff.push_back((int64_t)reads.size());
    }
    reads.push_back(0);                                            // (never a null pointer)
    dnas_fastseqs_free(fs);
    dnas_cluster_stats st;
    check(dnas_clusterer_add(h, n, reads.data(), readOff.data(), &st, nullptr));
    if (o.verbose >= 3)
      std::cerr << "Read clustering: " << file << ": " << n << " reads, " << st.candidates << " of " << st.pairs << " pairs scored, " << st.edges
                << " edges" << std::endl;
  }
  const int64_t n = dnas_clusterer_reads(h);
  std::vector<int64_t> root((size_t)n + 1), cluster((size_t)n + 1);
  std::vector<uint8_t> strand((size_t)n + 1), status((size_t)n + 1);
  dnas_cluster_stats st;
  check(dnas_clusterer_result(h, root.data(), cluster.data(), strand.data(), status.data(), nullptr, nullptr, nullptr, nullptr, &st, nullptr));
  dnas_clusterer_destroy(h);
  if (o.verbose >= 3)
    std::cerr << "Read clustering: " << st.clusters << " clusters; " << st.candidates << " of " << st.pairs << " pairs scored, " << st.edges
              << " edges, " << st.strand_conflicts << " strand conflicts" << std::endl;
  std::vector<std::string> names;
  for (int64_t i = 0; i < n; ++i) names.push_back("cluster" + std::to_string(cluster[(size_t)i]));
  return names;
}

// --outer-code n,k,L
struct OuterCode {
  int n = 0, k = 0, L = 0;
};
OuterCode parseOuterCode(const Options& o) {
  OuterCode c;
  char tail = 0;
  if (sscanf(o.outerCode.c_str(), "%d,%d,%d%c", &c.n, &c.k, &c.L, &tail) != 3) die("--outer-code takes n,k,L");
  return c;
}

// --outer-decode: the messages of a -V run, each a record when it decodes to 4 + L bytes with a matching CRC -> the file, and
// the report on stdout.
struct OuterSink {
  OuterCode code;
  std::vector<uint8_t> bytes;
  std::vector<int64_t> off{0};
  std::vector<double> weights;
  void add(const std::string& symbols, double weight) {
    uint8_t* b = nullptr;
    size_t nb = 0;
    if (!symbols.empty()) {
      check(dnas_symbols_to_bytes(symbols.data(), symbols.size(), &b, &nb));
      bytes.insert(bytes.end(), b, b + nb);
      dnas_free(b);
    }
    off.push_back((int64_t)bytes.size());
    weights.push_back(weight);
  }
  void finish(const Options& o) {
    const int64_t B = o.outerBlocks, slots = B * code.n;
    bytes.push_back(0);                                            // (never a null pointer)
    weights.push_back(0);
    std::vector<uint8_t> present((size_t)slots + 1), columns((size_t)(B * code.L) + 1);
    std::vector<int32_t> fixed((size_t)slots + 1);
    uint8_t* data = nullptr;
    int64_t len = 0, nRanges = 0, *ranges = nullptr;
    int32_t status = 0;
    dnas_outer_stats st;
    const bool host = dnas_device_count() <= 0;
    if (host) std::cerr << "No GPU: the outer code runs as the host statement" << std::endl;
    check(dnas_outer_decode((int64_t)off.size() - 1, bytes.data(), off.data(), weights.data(), code.n, code.k, code.L, B, o.device, host, &data,
                            &len, &status, present.data(), columns.data(), fixed.data(), &ranges, &nRanges, &st));
    std::ofstream out(o.outerDecode, std::ios::binary);
    if (!out) die("Cannot write " + o.outerDecode);
    out.write((const char*)data, (std::streamsize)len);
    static const char* const names[] = {"ok", "damaged", "no-length", "bad-length"};
    std::ostringstream js;
    js << "{\n \"status\": \"" << names[status] << "\",\n \"bytes\": " << len << ",\n \"blocks\": " << B << ",\n \"records\": " << st.records
       << ",\n \"dropped\": " << st.dropped << ",\n \"conflicts\": " << st.conflicts << ",\n \"ties\": " << st.ties << ",\n \"erased\": "
       << st.erased << ",\n \"columnsOk\": " << st.columns_ok << ",\n \"columnsCorrected\": " << st.columns_corrected
       << ",\n \"columnsFailed\": " << st.columns_failed << ",\n \"present\": [ ";
    for (int64_t b = 0; b < B; ++b) {
      int count = 0;
      for (int p = 0; p < code.n; ++p) count += present[(size_t)(b * code.n + p)];
      js << (b ? ", " : "") << count;
    }
    js << " ],\n \"fixed\": [ ";
    bool first = true;
    for (int64_t s = 0; s < slots; ++s)
      if (fixed[(size_t)s]) {
        js << (first ? "" : ", ") << "[ " << s << ", " << fixed[(size_t)s] << " ]";
        first = false;
      }
    js << " ],\n \"failedRanges\": [ ";
    for (int64_t q = 0; q < nRanges; ++q) js << (q ? ", " : "") << "[ " << ranges[2 * q] << ", " << ranges[2 * q + 1] << " ]";
    js << " ]\n}\n";
    std::cout << js.str();
    dnas_free(data);
    dnas_free(ranges);
  }
};

}  // namespace

int main(int argc, char** argv) {
  const Options o = parse(argc, argv);
  if (o.help) { std::cout << kHelp << "\n"; return 1; }
  if (o.length > 31) die("Maximum context is 31 bases");
  if (o.bothStrands && o.reverseStrand) die("--both-strands and --reverse-strand exclude each other");
  if ((o.bothStrands || o.reverseStrand) &&
      (o.decodeViterbi.empty() || !o.encodeFile.empty() || !o.decodeFile.empty() || !o.encodeString.empty() || !o.decodeString.empty() ||
       !o.encodeBits.empty() || !o.decodeBits.empty() || !o.fitError.empty() || !o.errorCounts.empty()))
    die("--both-strands and --reverse-strand go with -V [ --decode-viterbi ] only");
  if (o.clusterPolishGiven && (o.decodeViterbi.empty() || (o.clusterFile.empty() && !o.clusterAuto)))
    die("--cluster-polish goes with -V [ --decode-viterbi ] and --cluster-file or --cluster-auto only");
  if (o.clusterPolish < 0) die("--cluster-polish must be at least 0");
  if (o.clusterScoreGiven && (o.decodeViterbi.empty() || (o.clusterFile.empty() && !o.clusterAuto)))
    die("--cluster-score goes with -V [ --decode-viterbi ] and --cluster-file or --cluster-auto only");
  if (o.clusterScore != "viterbi" && o.clusterScore != "forward") die("--cluster-score must be viterbi or forward");
  if (!o.clusterFile.empty() &&
      (o.decodeViterbi.empty() || !o.encodeFile.empty() || !o.decodeFile.empty() || !o.encodeString.empty() || !o.decodeString.empty() ||
       !o.encodeBits.empty() || !o.decodeBits.empty() || !o.fitError.empty() || !o.errorCounts.empty()))
    die("--cluster-file goes with -V [ --decode-viterbi ] only");
  if (o.clusterAuto &&
      (o.decodeViterbi.empty() || !o.clusterFile.empty() || !o.clusterReads.empty() || !o.encodeFile.empty() || !o.decodeFile.empty() ||
       !o.encodeString.empty() || !o.decodeString.empty() || !o.encodeBits.empty() || !o.decodeBits.empty() || !o.fitError.empty() ||
       !o.errorCounts.empty()))
    die("--cluster-auto goes with -V [ --decode-viterbi ] only, and instead of --cluster-file");
  if (o.clusterMaxEditGiven && o.clusterReads.empty() && !o.clusterAuto) die("--cluster-max-edit goes with --cluster-reads or --cluster-auto only");
  if (!o.clusterAdd.empty() && o.clusterReads.empty()) die("--cluster-add goes with --cluster-reads only");
  if (o.clusterTable && o.clusterFile.empty() && !o.clusterAuto) die("--cluster-table goes with --cluster-file or --cluster-auto only");

  if (o.trimReads.empty() != o.trimPrimers.empty()) die("--trim-reads and --trim-primers go together");
  if (o.trimOptionGiven && o.trimReads.empty())
    die("--trim-max-offset, --trim-max-edit, --trim-anchors, --trim-min-payload and --trim-select go with --trim-reads only");
  if (o.simulateOptionGiven && o.simulateReads.empty())
    die("--simulate-coverage, --simulate-seed, --simulate-reverse, --simulate-shuffle and --simulate-stockholm go with --simulate-reads only");
  if (!o.trimReads.empty()) {
    trimPool(o);
    return 0;
  }
  if ((!o.outerEncode.empty() || !o.outerDecode.empty()) && o.outerCode.empty()) die("--outer-encode and --outer-decode need --outer-code n,k,L");
  if (!o.outerCode.empty() && o.outerEncode.empty() && o.outerDecode.empty()) die("--outer-code goes with --outer-encode or --outer-decode");
  if (!o.outerDecode.empty() && o.decodeViterbi.empty()) die("--outer-decode goes with -V [ --decode-viterbi ]");
  if (!o.outerDecode.empty() && o.outerBlocks < 1) die("--outer-decode needs --outer-blocks, at least 1");
  if (!o.outerEncode.empty() && !o.outerDecode.empty()) die("--outer-encode and --outer-decode exclude each other");
  OuterSink sink;
  if (!o.outerCode.empty()) sink.code = parseOuterCode(o);

  // error model: --error-file wins over the flags, `local` included (dnastore.cpp:115-130)
  dnas_mutator_params mut;
  if (!o.errorFile.empty()) check(dnas_mutator_params_load_json(o.errorFile.c_str(), &mut));
  else check(dnas_mutator_params_from_flags(o.subProb, o.ivRatio, o.dupProb, o.delOpen, o.delExt, o.errorGlobal ? 1 : 0, o.length, &mut));

  if (!o.simulateReads.empty()) {
    simulatePool(o, mut);
    return 0;
  }

  const std::string& pairsFile = !o.fitPairs.empty() ? o.fitPairs : !o.countPairs.empty() ? o.countPairs
                                 : !o.profilePairs.empty() ? o.profilePairs : o.alignPairs;
  if (!pairsFile.empty() || !o.alignReads.empty()) {
    if ((int)!o.fitPairs.empty() + (int)!o.countPairs.empty() + (int)!o.profilePairs.empty() + (int)!o.alignPairs.empty() > 1)
      die("--align-pairs, --fit-pairs, --count-pairs and --profile-pairs exclude each other");
    if (pairsFile.empty() || o.alignReads.empty())
      die("--align-pairs, --fit-pairs, --count-pairs or --profile-pairs and --align-reads go together");
    if (o.profileAnchor != "start" && o.profileAnchor != "end") die("--profile-anchor must be start or end");
    if (o.alignBand < DNAS_ALIGN_FULL) die("--align-band must be -1 (the full matrix) or at least 0");
    dnas_fastseqs *fa = nullptr, *fr = nullptr;
    check(dnas_fastseqs_read(pairsFile.c_str(), &fa));
    check(dnas_fastseqs_read(o.alignReads.c_str(), &fr));
    const int64_t nIn = dnas_fastseqs_count(fa), n = dnas_fastseqs_count(fr);
    if (nIn != n && nIn != 1)
      die(std::to_string(nIn) + " originals for " + std::to_string(n) + " reads: the files pair by order (or one original with all reads)");
    std::vector<int8_t> ins, outs;
    std::vector<int64_t> inOff(1, 0), outOff(1, 0);
    std::vector<const char*> namesIn, namesOut;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t j = nIn == 1 ? 0 : i;
      tokens(dnas_fastseqs_name(fa, j), dnas_fastseqs_seq(fa, j), ins);
      tokens(dnas_fastseqs_name(fr, i), dnas_fastseqs_seq(fr, i), outs);
      inOff.push_back((int64_t)ins.size());
      outOff.push_back((int64_t)outs.size());
      namesIn.push_back(dnas_fastseqs_name(fa, j));
      namesOut.push_back(dnas_fastseqs_name(fr, i));
    }
    if (!o.alignPairs.empty()) {
      printAlignments(o, mut, ins, inOff, outs, outOff, namesIn, namesOut);
    } else if (!o.profilePairs.empty()) {
      ins.push_back(0); outs.push_back(0);                         // (never a null pointer)
      int64_t nPos = 0;
      for (int64_t i = 0; i < n; ++i) nPos = std::max(nPos, inOff[(size_t)i + 1] - inOff[(size_t)i] + 1);
      const size_t planes = (size_t)(DNAS_PROFILE_SUM_DUP + mut.n_len);
      std::vector<double> profile(planes * (size_t)nPos + 1), pairLl((size_t)n + 1);
      std::vector<int64_t> coverage((size_t)nPos + 1);
      std::vector<uint8_t> status((size_t)n + 1);
      check(dnas_pair_profiles(&mut, o.alignBand, n, ins.data(), inOff.data(), outs.data(), outOff.data(), nullptr, o.device, 0,
                               o.profileAnchor == "end" ? DNAS_PROFILE_FROM_END : DNAS_PROFILE_FROM_START, nPos, profile.data(),
                               coverage.data(), nullptr, pairLl.data(), status.data(), nullptr));
      // laid out as --count-pairs prints its counts, every number with the digits that read back to the same double
      std::ostringstream js;
      js.precision(17);
      const auto plane = [&](int j) {
        js << "[ ";
        for (int64_t p = 0; p < nPos; ++p) js << (p ? ", " : "") << profile[(size_t)j * (size_t)nPos + (size_t)p];
        js << " ]";
      };
      js << "{\n \"anchor\": \"" << o.profileAnchor << "\",\n \"positions\": " << nPos << ",\n \"coverage\": [ ";
      for (int64_t p = 0; p < nPos; ++p) js << (p ? ", " : "") << coverage[(size_t)p];
      js << " ]";
      const char* const names[] = {"same", "transition", "transversion", "delOpen", "delExtend"};
      for (int j = 0; j < DNAS_PROFILE_SUM_DUP; ++j) {
        js << ",\n \"" << names[j] << "\": ";
        plane(j);
      }
      js << ",\n \"dup\": [ ";
      for (int k = 0; k < mut.n_len; ++k) {
        js << (k ? ", " : "");
        plane(DNAS_PROFILE_SUM_DUP + k);
      }
      js << " ]\n}\n";
      std::cout << js.str();
    } else {
      ins.push_back(0); outs.push_back(0);                         // (never a null pointer)
      char buf[16384];
      if (!o.fitPairs.empty()) {                                   // as --fit-error prints its fit
        dnas_mutator_params fit;
        check(dnas_baum_welch_pairs(&mut, o.alignBand, n, ins.data(), inOff.data(), outs.data(), outOff.data(), nullptr, o.device, 0, 0,
                                    &fit, nullptr, nullptr, nullptr, nullptr));
        check(dnas_mutator_params_json(&fit, buf, sizeof buf));
      } else {                                                     // as --error-counts prints its counts
        std::vector<double> counts(21 + mut.n_len), pairLl((size_t)n + 1);
        std::vector<uint8_t> status((size_t)n + 1);
        double ll = 0;
        dnas_counts_stats st;
        check(dnas_pair_counts(&mut, o.alignBand, n, ins.data(), inOff.data(), outs.data(), outOff.data(), nullptr, o.device, 0,
                               counts.data(), &ll, nullptr, pairLl.data(), nullptr, status.data(), &st));
        if (o.verbose >= 3)
          std::cerr << "Pair counts: " << st.cells << " cells, " << st.waves << " waves, " << st.scratch_bytes << " bytes of scratch, kernel "
                    << st.kernel_ms << " ms, log-likelihood " << ll << std::endl;
        check(dnas_mutator_counts_json(counts.data(), mut.n_len, buf, sizeof buf));
      }
      std::cout << buf;
    }
    dnas_fastseqs_free(fa);
    dnas_fastseqs_free(fr);
    return 0;
  }

  if (!o.assignReads.empty() || !o.assignOriginals.empty()) {
    if (o.assignReads.empty() || o.assignOriginals.empty()) die("--assign-reads and --assign-originals go together");
    if (o.alignBand < DNAS_ALIGN_FULL) die("--align-band must be -1 (the full matrix) or at least 0");
    const int mode = o.assignStrands == "forward" ? DNAS_STRAND_FORWARD : o.assignStrands == "reverse" ? DNAS_STRAND_REVERSE
                     : o.assignStrands == "both" ? DNAS_STRAND_BOTH : -1;
    if (mode < 0) die("--assign-strands must be forward, reverse or both");
    dnas_fastseqs *fa = nullptr, *fr = nullptr;
    check(dnas_fastseqs_read(o.assignOriginals.c_str(), &fa));
    check(dnas_fastseqs_read(o.assignReads.c_str(), &fr));
    const int64_t K = dnas_fastseqs_count(fa), n = dnas_fastseqs_count(fr);
    std::vector<int8_t> origs, reads;
    std::vector<int64_t> origOff(1, 0), readOff(1, 0);
    for (int64_t k = 0; k < K; ++k) {
      tokens(dnas_fastseqs_name(fa, k), dnas_fastseqs_seq(fa, k), origs);
      origOff.push_back((int64_t)origs.size());
    }
    for (int64_t i = 0; i < n; ++i) {
      tokens(dnas_fastseqs_name(fr, i), dnas_fastseqs_seq(fr, i), reads);
      readOff.push_back((int64_t)reads.size());
    }
    origs.push_back(0); reads.push_back(0);                          // (never a null pointer)
    std::vector<int64_t> original((size_t)n + 1);
    std::vector<uint8_t> strand((size_t)n + 1), status((size_t)n + 1);
    std::vector<double> score((size_t)n + 1), second((size_t)n + 1);
    dnas_assign_stats st;
    check(dnas_assign_reads(&mut, o.alignBand, K, origs.data(), origOff.data(), n, reads.data(), readOff.data(), mode, nullptr, nullptr,
                            o.device, original.data(), strand.data(), score.data(), second.data(), status.data(), nullptr, &st));
    if (o.verbose >= 3)
      std::cerr << "Read assignment: " << st.items << " items, " << st.cells << " cells in " << st.chunks << " chunks, score "
                << st.score_ms << " ms, fold " << st.fold_ms << " ms" << std::endl;
    // the log-odds over the runner-up original; an unassigned read has none
    auto margin = [&](int64_t i) { return original[(size_t)i] < 0 ? -HUGE_VAL : score[(size_t)i] - second[(size_t)i]; };
    if (!o.assignStockholm) {
      char num[64];
      for (int64_t i = 0; i < n; ++i) {
        std::cout << dnas_fastseqs_name(fr, i) << "\t";
        if (original[(size_t)i] < 0) std::cout << "*";
        else std::cout << dnas_fastseqs_name(fa, original[(size_t)i]);
        std::cout << "\t" << (strand[(size_t)i] ? "-" : "+");
        snprintf(num, sizeof num, "\t%.17g\t%.17g\n", score[(size_t)i], margin(i));
        std::cout << num;
      }
    } else {
      std::vector<int8_t> ins, outs;
      std::vector<int64_t> inOff(1, 0), outOff(1, 0);
      std::vector<const char*> namesIn, namesOut;
      for (int64_t i = 0; i < n; ++i) {
        const char* name = dnas_fastseqs_name(fr, i);
        if (original[(size_t)i] < 0 || !(margin(i) >= o.assignMinMargin)) {
          std::cerr << "Not assigned: " << name << ": "
                    << (status[(size_t)i] == DNAS_ASSIGN_NO_CANDIDATES ? "there are no originals"
                        : status[(size_t)i] == DNAS_ASSIGN_NO_PATH ? "the error model has no path from any original"
                        : "the margin over the runner-up original is below --assign-min-margin") << std::endl;
          continue;
        }
        const int64_t k = original[(size_t)i], O = readOff[(size_t)i + 1] - readOff[(size_t)i];
        ins.insert(ins.end(), origs.begin() + origOff[(size_t)k], origs.begin() + origOff[(size_t)k + 1]);
        const int8_t* const b = reads.data() + readOff[(size_t)i];
        for (int64_t j = 0; j < O; ++j) outs.push_back(strand[(size_t)i] ? (int8_t)(3 - b[O - 1 - j]) : b[j]);
        inOff.push_back((int64_t)ins.size());
        outOff.push_back((int64_t)outs.size());
        namesIn.push_back(dnas_fastseqs_name(fa, k));
        namesOut.push_back(name);
      }
      printAlignments(o, mut, ins, inOff, outs, outOff, namesIn, namesOut);
    }
    dnas_fastseqs_free(fa);
    dnas_fastseqs_free(fr);
    return 0;
  }

  if (!o.clusterReads.empty() && !o.clusterAdd.empty()) {
    std::vector<std::string> files(1, o.clusterReads);
    files.insert(files.end(), o.clusterAdd.begin(), o.clusterAdd.end());
    for (const std::string& name : clusterNamesBatched(o, mut, files)) std::cout << name << "\n";
    return 0;
  }
  if (!o.clusterReads.empty()) {
    dnas_fastseqs* fs = nullptr;
    check(dnas_fastseqs_read(o.clusterReads.c_str(), &fs));
    for (const std::string& name : clusterNames(o, mut, fs)) std::cout << name << "\n";
    dnas_fastseqs_free(fs);
    return 0;
  }

  if (!o.fitError.empty() || !o.errorCounts.empty()) {
    dnas_pairs* db = nullptr;
    check(dnas_stockholm_read((!o.fitError.empty() ? o.fitError : o.errorCounts).c_str(), &db));
    const dnas_pairs_view* v = dnas_pairs_get(db);
    if (o.verbose >= 3) {                                          // how many devices the E-step handle spans
      dnas_fb* fb = nullptr;
      check(dnas_fb_create(o.device, &fb));
      std::cerr << "E-step devices: " << dnas_fb_devices(fb) << std::endl;
      dnas_fb_destroy(fb);
    }
    char buf[16384];
    if (!o.fitError.empty()) {                                     // dnastore.cpp:135-140
      dnas_mutator_params fit;
      check(dnas_baum_welch(&mut, o.strictGuides, v->n_pairs, v->in_seqs, v->in_off, v->out_seqs, v->out_off, v->cm_in, v->cm_in_off,
                            v->cm_out, v->cm_out_off, o.device, &fit, nullptr));
      check(dnas_mutator_params_json(&fit, buf, sizeof buf));
    } else {                                                       // dnastore.cpp:142-146
      std::vector<double> counts(21 + mut.n_len);
      double ll = 0;
      check(dnas_fwdback_estep(&mut, o.strictGuides, v->n_pairs, v->in_seqs, v->in_off, v->out_seqs, v->out_off, v->cm_in, v->cm_in_off,
                               v->cm_out, v->cm_out_off, o.device, counts.data(), &ll, nullptr));
      check(dnas_mutator_counts_json(counts.data(), mut.n_len, buf, sizeof buf));
    }
    std::cout << buf;
    dnas_pairs_free(db);
    return 0;
  }

  // primary machine
  dnas_machine* machine = nullptr;
  if (!o.loadMachine.empty()) {
    check(dnas_machine_load_json(o.loadMachine.c_str(), &machine));
  } else {
    const char* canon = getenv("DNASTORE_L4C4");
    if (o.length == 4 && o.controls == 4 && canon) check(dnas_machine_load_json(canon, &machine));
    else die("this build does not contain the de Bruijn code builder: pass --load-machine (for -l 4 -c 4, set DNASTORE_L4C4 to data/l4c4.json)");
  }
  for (auto it = o.compose.rbegin(); it != o.compose.rend(); ++it) {   // right to left, dnastore.cpp:159-165
    dnas_machine *front = nullptr, *prod = nullptr;
    check(dnas_machine_load_json(it->c_str(), &front));
    check(dnas_machine_compose(front, machine, &prod));
    dnas_machine_free(front);
    dnas_machine_free(machine);
    machine = prod;
  }
  if (!o.saveMachine.empty()) {
    char* text = nullptr;
    size_t n = 0;
    check(dnas_machine_write_json(machine, &text, &n));
    if (o.saveMachine == "-") std::cout << text;
    else { std::ofstream out(o.saveMachine); out << text; }
    dnas_free(text);
  }

  char* text = nullptr;
  size_t n = 0;
  auto encodeOut = [&](int rc, const char* name) {
    check(rc);
    if (o.raw) std::cout << text << "\n";                           // FastaWriter with no header: one line
    else writeFasta(std::cout, name, text, false);
    dnas_free(text);
  };
  if (!o.outerEncode.empty()) {
    const std::string data = slurp(o.outerEncode, "Binary file");
    int64_t B = 0;
    uint8_t* records = nullptr;
    const bool host = dnas_device_count() <= 0;
    if (host) std::cerr << "No GPU: the outer code runs as the host statement" << std::endl;
    check(dnas_outer_encode((const uint8_t*)data.data(), (int64_t)data.size(), sink.code.n, sink.code.k, sink.code.L, o.device, host, &B, &records));
    const size_t rec = 4 + (size_t)sink.code.L;
    for (int64_t s = 0; s < B * sink.code.n; ++s) {
      check(dnas_encode_bytes(machine, records + (size_t)s * rec, rec, &text, &n));
      writeFasta(std::cout, ("s" + std::to_string(s)).c_str(), text, o.raw);
      dnas_free(text);
    }
    dnas_free(records);
    std::cerr << "Outer code: " << B << " blocks, " << B * sink.code.n << " strands (--outer-blocks " << B << ")" << std::endl;
  } else if (!o.encodeFile.empty()) {
    const std::string data = slurp(o.encodeFile, "Binary file");
    encodeOut(dnas_encode_bytes(machine, (const uint8_t*)data.data(), data.size(), &text, &n), o.encodeFile.c_str());
  } else if (!o.decodeFile.empty()) {                               // dnastore.cpp:188-193
    dnas_fastseqs* fs = nullptr;
    check(dnas_fastseqs_read(o.decodeFile.c_str(), &fs));
    for (int64_t i = 0; i < dnas_fastseqs_count(fs); ++i) {
      const char* seq = dnas_fastseqs_seq(fs, i);
      check(dnas_decode_exact(machine, seq, strlen(seq), &text, &n));
      uint8_t* bytes = nullptr;
      size_t nb = 0;
      check(dnas_symbols_to_bytes(text, n, &bytes, &nb));
      std::cout.write((const char*)bytes, (std::streamsize)nb);
      dnas_free(bytes);
      dnas_free(text);
    }
    dnas_fastseqs_free(fs);
  } else if (!o.encodeString.empty()) {
    encodeOut(dnas_encode_bytes(machine, (const uint8_t*)o.encodeString.data(), o.encodeString.size(), &text, &n), "ASCII_string");
  } else if (!o.decodeString.empty()) {
    check(dnas_decode_exact(machine, o.decodeString.data(), o.decodeString.size(), &text, &n));
    uint8_t* bytes = nullptr;
    size_t nb = 0;
    check(dnas_symbols_to_bytes(text, n, &bytes, &nb));
    std::cout.write((const char*)bytes, (std::streamsize)nb);
    dnas_free(bytes);
    dnas_free(text);
  } else if (!o.encodeBits.empty()) {
    encodeOut(dnas_encode_symbols(machine, o.encodeBits.data(), o.encodeBits.size(), &text, &n), "bit_string");
  } else if (!o.decodeBits.empty()) {
    check(dnas_decode_exact(machine, o.decodeBits.data(), o.decodeBits.size(), &text, &n));
    std::cout << text << "\n";
    dnas_free(text);
  } else if (!o.decodeViterbi.empty() && (!o.clusterFile.empty() || o.clusterAuto)) {  // clusters of reads -> one message each
    if (o.alignBand < DNAS_ALIGN_FULL) die("--align-band must be -1 (the full matrix) or at least 0");
    if (o.device < 0) die("--cluster-file and --cluster-auto decode on one GPU: --device must name it");
    dnas_fastseqs* fs = nullptr;
    check(dnas_fastseqs_read(o.decodeViterbi.c_str(), &fs));
    const int64_t nReads = dnas_fastseqs_count(fs);
    std::vector<std::string> labels;
    if (o.clusterAuto) {
      labels = clusterNames(o, mut, fs);
    } else {
      std::ifstream in(o.clusterFile);
      if (!in) die("Cluster file not found");
      for (std::string line; std::getline(in, line);) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        labels.push_back(line);
      }
    }
    if ((int64_t)labels.size() != nReads)
      die(std::to_string(labels.size()) + " cluster names for " + std::to_string(nReads) + " reads: --cluster-file has one line per read");
    // the clusters in order of first appearance, the reads grouped by cluster in file order
    std::vector<std::string> names;
    std::vector<std::vector<int64_t>> members;
    std::map<std::string, size_t> clusterOf;
    for (int64_t i = 0; i < nReads; ++i) {
      const auto at = clusterOf.emplace(labels[(size_t)i], names.size());
      if (at.second) { names.push_back(labels[(size_t)i]); members.emplace_back(); }
      members[at.first->second].push_back(i);
    }
    const int64_t nClusters = (int64_t)names.size();
    std::vector<int8_t> toks;
    std::vector<uint64_t> readOff(1, 0), outOff(1, 0), consSymOff(1, 0);
    std::vector<int64_t> clusterOff(1, 0);
    for (const auto& mine : members) {
      size_t first = 0, longest = 0;
      for (int64_t i : mine) {
        tokens(dnas_fastseqs_name(fs, i), dnas_fastseqs_seq(fs, i), toks);
        const size_t mineLen = toks.size() - readOff.back();
        if (i == mine.front()) first = mineLen;
        longest = std::max(longest, mineLen);
        outOff.push_back(outOff.back() + 4 * mineLen + 64);
        readOff.push_back(toks.size());
      }
      clusterOff.push_back((int64_t)readOff.size() - 1);
      consSymOff.push_back(consSymOff.back() + 4 * (first + 2 * (size_t)o.clusterPolish * longest) + 64);   // what a consensus read can grow to
    }
    toks.push_back(0);                                               // (never a null pointer)
    dnas_flat* flat = nullptr;
    dnas_model* model = nullptr;
    check(dnas_flatten(machine, &mut, &flat));
    check(dnas_model_create(dnas_flat_view(flat), o.device, 0, &model));
    const size_t n1 = (size_t)nReads + 1, c1 = (size_t)nClusters + 1;
    std::vector<char> sym, consSym;                                  // (sized in the loop below)
    std::vector<uint32_t> len(n1);
    std::vector<double> ll(n1), total(c1), second(c1);
    std::vector<uint8_t> status(n1), strand(n1), clusterStatus(c1);
    std::vector<int64_t> proposer(c1);
    std::vector<int32_t> nCand(c1), votes(c1);
    dnas_consensus_stats st;
    std::vector<uint8_t> source(c1), consStatus(c1);
    std::vector<int64_t> consOff(c1);
    std::vector<uint32_t> consLen(c1);
    std::vector<double> consLl(c1);
    int8_t* consSeqs = nullptr;
    const bool forwardScore = o.clusterScore == "forward";
    const int strandMode = o.bothStrands ? DNAS_STRAND_BOTH : o.reverseStrand ? DNAS_STRAND_REVERSE : DNAS_STRAND_FORWARD;
    std::vector<double> confidence(c1);
    // The slots are this tool's own, 4 L + 64 symbols for L bases: a guess, since a walk decodes a symbol per state it passes.  A
    // read (or consensus read) that overflowed its slot has left there the length it needs; the clusters are then decoded once
    // more with those slots, so that every candidate is there to be scored.
    auto growSlots = [](const std::vector<char>& buf, std::vector<uint64_t>& off, const std::vector<uint8_t>& st, int64_t n) {
      bool grown = false;
      std::vector<uint64_t> cap((size_t)n);
      for (int64_t i = 0; i < n; ++i) {
        cap[(size_t)i] = off[(size_t)i + 1] - off[(size_t)i];
        const uint64_t need = st[(size_t)i] == DNAS_READ_OUT_OVERFLOW ? dnas_slot_needed(buf.data() + off[(size_t)i], cap[(size_t)i]) : 0;
        if (need > cap[(size_t)i]) { cap[(size_t)i] = need; grown = true; }
      }
      for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + cap[(size_t)i];
      return grown;
    };
    for (int attempt = 0;; ++attempt) {
      sym.assign((size_t)outOff.back() + 1, 0);
      consSym.assign((size_t)consSymOff.back() + 1, 0);
      dnas_free(consSeqs);
      consSeqs = nullptr;
      if (forwardScore)
        check(dnas_viterbi_clusters_scored(model, machine, &mut, o.alignBand, nReads, readOff.data(), (const uint8_t*)toks.data(),
                                           clusterOff.data(), nClusters, strandMode, o.clusterPolish, sym.data(), outOff.data(), len.data(),
                                           ll.data(), status.data(), strand.data(), proposer.data(), total.data(), second.data(), nCand.data(),
                                           votes.data(), clusterStatus.data(), source.data(), &consSeqs, consOff.data(), consSym.data(),
                                           consSymOff.data(), consLen.data(), consLl.data(), consStatus.data(), DNAS_SCORE_FORWARD,
                                           confidence.data(), &st));
      else
        check(dnas_viterbi_clusters_ex(model, machine, &mut, o.alignBand, nReads, readOff.data(), (const uint8_t*)toks.data(), clusterOff.data(),
                                       nClusters, strandMode, o.clusterPolish, sym.data(), outOff.data(), len.data(), ll.data(), status.data(),
                                       strand.data(), proposer.data(), total.data(), second.data(), nCand.data(), votes.data(),
                                       clusterStatus.data(), source.data(), &consSeqs, consOff.data(), consSym.data(), consSymOff.data(),
                                       consLen.data(), consLl.data(), consStatus.data(), &st));
      if (attempt > 0) break;
      const bool readsGrown = growSlots(sym, outOff, status, nReads);
      const bool consGrown = o.clusterPolish > 0 && growSlots(consSym, consSymOff, consStatus, nClusters);
      if (!readsGrown && !consGrown) break;
    }
    dnas_free(consSeqs);
    if (o.verbose >= 3)
      std::cerr << "Viterbi fill: " << dnas_model_tier(model) << "; consensus: " << st.candidates << " candidates, " << st.encode_failures
                << " messages not encodable, " << st.items << " items, " << st.cells << " cells in " << st.chunks << " chunks, score "
                << st.score_ms << " ms, fold " << st.fold_ms << " ms" << std::endl;
    for (int64_t c = 0; c < nClusters; ++c) {
      const int64_t r = proposer[(size_t)c];
      const bool fromCons = source[(size_t)c] != 0;
      const std::string seq = fromCons ? std::string(consSym.data() + consSymOff[(size_t)c], consLen[(size_t)c])
                              : r < 0 ? std::string() : std::string(sym.data() + outOff[(size_t)r], len[(size_t)r]);
      if (r < 0 && !fromCons)
        std::cerr << "No consensus for " << names[(size_t)c] << ": "
                  << (clusterStatus[(size_t)c] == DNAS_CONSENSUS_NO_CANDIDATES ? "none of its reads decoded to a message"
                      : clusterStatus[(size_t)c] == DNAS_CONSENSUS_NO_READS ? "it has no reads"
                      : "the error model has no path from any candidate to all of its reads") << std::endl;
      if (!o.outerDecode.empty()) {
        sink.add(seq, forwardScore ? confidence[(size_t)c] : 1.0);
      } else if (o.clusterTable) {
        char num[64];
        snprintf(num, sizeof num, "\t%.17g\t%.17g\t", total[(size_t)c], r < 0 && !fromCons ? -HUGE_VAL : total[(size_t)c] - second[(size_t)c]);
        std::cout << names[(size_t)c] << "\t" << members[(size_t)c].size() << "\t" << nCand[(size_t)c] << "\t" << votes[(size_t)c] << num << seq;
        if (o.clusterPolish > 0) std::cout << "\t" << (int)source[(size_t)c];
        if (forwardScore) {
          snprintf(num, sizeof num, "\t%.17g", confidence[(size_t)c]);
          std::cout << num;
        }
        std::cout << "\n";
      } else {
        writeFasta(std::cout, names[(size_t)c].c_str(), seq, o.raw);
      }
    }
    if (!o.outerDecode.empty()) sink.finish(o);
    dnas_model_destroy(model);
    dnas_flat_free(flat);
    dnas_fastseqs_free(fs);
  } else if (!o.decodeViterbi.empty()) {                            // dnastore.cpp:217-223
    dnas_decoded* dec = nullptr;
    const bool strands = o.bothStrands || o.reverseStrand;
    if (strands)
      check(dnas_decode_fastseqs_strands(o.decodeViterbi.c_str(), machine, &mut, o.device, o.verbose >= 3,
                                         o.bothStrands ? DNAS_STRAND_BOTH : DNAS_STRAND_REVERSE, &dec));
    else
      check(dnas_decode_fastseqs_ex(o.decodeViterbi.c_str(), machine, &mut, o.device, o.verbose >= 3, &dec));
    if (o.verbose >= 3) {
      std::cerr << "Viterbi fill: " << dnas_decoded_tier(dec) << "; devices: " << dnas_decoded_devices(dec);
      if (strands) std::cerr << "; strands: " << (o.bothStrands ? "the likelier of both" : "reverse");
      std::cerr << std::endl;
    }
    for (int64_t i = 0; i < dnas_decoded_count(dec); ++i) {
      const std::string seq = dnas_decoded_seq(dec, i);
      if (o.verbose >= 3 && strands)                                 // (event positions then count along the decoded orientation)
        std::cerr << "Strand of " << dnas_decoded_name(dec, i) << ": " << (dnas_decoded_strand(dec, i) ? "reverse" : "forward") << std::endl;
      if (o.verbose >= 3) {                                          // what the traceback found (viterbi.cpp:266-293)
        const uint64_t* ev = nullptr;
        const int64_t ne = dnas_decoded_events(dec, i, &ev);
        static const char base[] = "ACGT";
        for (int64_t k = 0; k < ne; ++k) {
          const unsigned kind = (unsigned)(ev[k] >> 62), pos = (unsigned)((ev[k] >> 32) & 0x3fffffffu), pay = (unsigned)(ev[k] & 0xffffffffu);
          if (kind == 1) std::cerr << "Substitution at " << pos << ": " << base[(pay >> 2) & 3] << " -> " << base[pay & 3] << std::endl;
          else if (kind == 2) std::cerr << "Deletion between " << (long)pos - 1 << " and " << pos << ": " << base[pay & 3] << std::endl;
          else if (kind == 3) {
            std::string dup;
            const unsigned cnt = pay >> 26;
            for (unsigned q = 0; q < cnt; ++q) dup.push_back(base[(pay >> (2 * (cnt - 1 - q))) & 3]);
            std::cerr << "Duplication at " << pos << ": " << dup << std::endl;
          }
        }
      }
      if (seq.empty()) std::cerr << "No valid Viterbi decoding found" << std::endl;   // viterbi.cpp:198-201
      if (!o.outerDecode.empty()) sink.add(seq, 1.0);
      else writeFasta(std::cout, dnas_decoded_name(dec, i), seq, o.raw);
    }
    if (!o.outerDecode.empty()) sink.finish(o);
    dnas_decoded_free(dec);
  }
  dnas_machine_free(machine);
  return 0;
}
