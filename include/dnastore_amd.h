/*
 * dnastore_amd.h -- C ABI of the MI355X-native error decoder for ihh/dnastore.
 *
 * The reference has no FFI/plugin boundary: its Viterbi path is the C++ function
 *   vguard<FastSeq> decodeFastSeqs(const char*, const Machine&, const MutatorParams&)
 * (reference src/viterbi.h:108, src/viterbi.cpp:306-320) called from one arm of main
 * (t/dnastore.cpp:217-223).  This header is the boundary a maintainer would bind in its
 * place: plain pointers and sizes, opaque handles, int status returns, no exceptions,
 * no torch types.  Each entry point names the reference interface it replaces.
 *
 * Threading: a handle is thread-compatible (one host thread / one GPU per handle).
 * Every function returns DNAS_OK (0) or a negative DNAS_E_* code; dnas_last_error()
 * returns the message of the calling thread's last failure.
 */
#ifndef DNASTORE_AMD_H
#define DNASTORE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNAS_OK 0
#define DNAS_E_INVALID (-1)   /* bad argument                                              */
#define DNAS_E_IO (-2)        /* file not found / unreadable  (reference: Fail -> exit(1))  */
#define DNAS_E_PARSE (-3)     /* malformed JSON / FASTA / contexts (verifyContexts)         */
#define DNAS_E_CYCLIC (-4)    /* "Transducer is cyclic, can't toposort" (trans.cpp:631-632) */
#define DNAS_E_NOT_DNA (-5)   /* "Not a DNA-outputting machine" (viterbi.cpp:27-28)         */
#define DNAS_E_BAD_BASE (-6)  /* non-ACGT read character (fastseq.cpp:30-35)                */
#define DNAS_E_DEVICE (-7)    /* HIP runtime failure / no GPU / extension not built         */
#define DNAS_E_NOMEM (-8)
#define DNAS_E_UNSUPPORTED (-9)

/* per-read status written by dnas_viterbi_batch */
#define DNAS_READ_OK 0
#define DNAS_READ_NO_PATH 1        /* loglike == -inf: empty string, "No valid Viterbi decoding found" (viterbi.cpp:198-201) */
#define DNAS_READ_OUT_OVERFLOW 2   /* decoded string longer than the caller's slot            */
#define DNAS_READ_TRACEBACK_FAIL 3 /* checkBest assertion (viterbi.cpp:230-237)               */

typedef struct dnas_machine dnas_machine; /* Machine, reference src/trans.h:82-126 */
typedef struct dnas_model dnas_model;     /* device-resident MachineScores + MutatorScores + InputModel */

/* MutatorParams, reference src/mutator.h:9-31 */
typedef struct dnas_mutator_params {
  double p_del_open, p_del_extend, p_tan_dup, p_transition, p_transversion;
  int32_t n_len;        /* pLen.size() = maxDupLen(), 0..32 (more: DNAS_E_UNSUPPORTED) */
  int32_t local;        /* 1 = local (partial reads allowed), 0 = --error-global */
  double p_len[32];
} dnas_mutator_params;

/*
 * The flattened model: everything ViterbiMatrix derives from (Machine, MutatorParams)
 * before touching a read -- InputModel (viterbi.cpp:6-14,309-310), MachineScores
 * (viterbi.cpp:23-60), MutatorScores (mutator.cpp:56-75), decoderToposort
 * (trans.cpp:604-634) -- as flat CSR arrays.  Edge order inside every row is the
 * reference's enumeration order (ascending source state, then transition order), which
 * is the traceback tie-break order.  All pointers are owned by the dnas_flat handle.
 */
typedef struct dnas_flat_model {
  int32_t n_states;      /* N                                                   */
  int32_t max_dup_len;   /* D = min(maxLeftContext, P), viterbi.cpp:63          */
  int32_t n_len;         /* P                                                   */
  int32_t local;
  int32_t n_emit, n_null;
  /* incoming edges per destination state */
  const int32_t *ein_ptr, *ein_src;   const double *ein_score; const uint8_t *ein_in, *ein_base;
  const int32_t *nin_ptr, *nin_src;   const double *nin_score; const uint8_t *nin_in;
  /* outgoing edges per source state */
  const int32_t *eout_ptr, *eout_dst; const double *eout_score;
  const int32_t *nout_ptr, *nout_dst; const double *nout_score;
  const uint8_t *mdl;                 /* [N]   maxDupLenAt, viterbi.h:104                      */
  const uint8_t *ctx;                 /* [N*D] ctx[j*D+k] = tanDupBase(j,k), viterbi.h:105     */
  const int32_t *topo;                /* [N]   decoderToposort order                           */
  double no_gap, del_open, del_extend, del_end, tan_dup;
  double sub[16];                     /* sub[base*4+observed]                                  */
  const double *len;                  /* [P]                                                   */
  char alphabet[64];                  /* inputAlphabet(Relaxed|Control|SEOF)                   */
  double sym_logp[128];               /* log P(input symbol), 0 where absent                   */
} dnas_flat_model;

typedef struct dnas_flat dnas_flat;

/* ---- host side: file formats (no GPU needed) ------------------------------------- */

/* Machine::fromFile / readJSON (trans.cpp:431-482). */
int dnas_machine_load_json(const char *path, dnas_machine **out);
int dnas_machine_parse_json(const char *text, size_t len, dnas_machine **out);
void dnas_machine_free(dnas_machine *m);
int32_t dnas_machine_n_states(const dnas_machine *m);
/* Machine::writeJSON (trans.cpp:402-429) into a malloc'd buffer the caller frees with dnas_free. */
int dnas_machine_write_json(const dnas_machine *m, char **out_text, size_t *out_len);

/* Exact encoder (reference Encoder<FastaWriter>, src/encoder.h:7-243): input symbols
 * ('^', '0', '1', '$', controls ...; SOF/EOF are added when missing, as the reference does)
 * or raw bytes (bits LSB first, encoder.h:222-231) -> DNA string, malloc'd, caller frees
 * with dnas_free.  Makes synthetic reads for bench.py and the parity tests. */
int dnas_encode_symbols(const dnas_machine *m, const char *symbols, size_t n_symbols, char **out_dna, size_t *out_len);
int dnas_encode_bytes(const dnas_machine *m, const uint8_t *bytes, size_t n_bytes, char **out_dna, size_t *out_len);

/* Machine::compose(first, second) (trans.cpp:505-602): first's output feeds second's input. */
int dnas_machine_compose(const dnas_machine *first, const dnas_machine *second, dnas_machine **out);

/* Exact decoder (reference Decoder<W>, src/decoder.h:7-191): DNA -> input symbols (malloc'd string),
 * and BinaryWriter (decoder.h:193-240): '0'/'1' symbols -> bytes, LSB first (malloc'd, *out_len bytes). */
int dnas_decode_exact(const dnas_machine *m, const char *dna, size_t n, char **out_symbols, size_t *out_len);
int dnas_symbols_to_bytes(const char *symbols, size_t n, uint8_t **out_bytes, size_t *out_len);

/* Error model from the CLI flags (t/dnastore.cpp:119-129): --error-sub-prob, --error-iv-ratio,
 * --error-dup-prob, --error-del-open, --error-del-ext, --error-global, --length. */
int dnas_mutator_params_from_flags(double sub_prob, double iv_ratio, double dup_prob, double del_open,
                                   double del_ext, int global, int length, dnas_mutator_params *out);
/* MutatorParams::fromFile (mutator.cpp:18-49), the --error-file format. */
int dnas_mutator_params_load_json(const char *path, dnas_mutator_params *out);

/* MachineScores + InputModel + MutatorScores + toposort, once per (machine, params). */
int dnas_flatten(const dnas_machine *m, const dnas_mutator_params *p, dnas_flat **out);
const dnas_flat_model *dnas_flat_view(const dnas_flat *f);
void dnas_flat_free(dnas_flat *f);

/* ---- device side ------------------------------------------------------------------ */

/* Upload the flattened model to GPU `device_id` and size the lattice arena.
 * arena_bytes = 0 picks a default (a fraction of free HBM). */
int dnas_model_create(const dnas_flat_model *fm, int device_id, size_t arena_bytes, dnas_model **out);
/* The same with options, "key=value,key=value" (NULL: none).  Keys: tier = A | B | C (force a fill kernel; failing
 * to provide it is then an error), cluster = work-groups per read for tier C, threads = 512 | 1024 per work-group
 * (default 1024 for tier A; tier C takes 512 when the machine then fits fewer work-groups), max_clusters, max_slots (reads per
 * fill launch), fill_overlap = 0 | 1 | 2 (tier A, calls of three or more fill launches: the launches go down two streams into a
 * ring of three arena slices, so that a launch's last round of work-groups shares the chip with the next launch.  1, the default:
 * when three batches fit the arena side by side, or the arena is the library's default -- the batches are then cut to a third of
 * it; 2: an arena_bytes of the caller's is cut in three as well; 0: never.  Results do not depend on it), cluster_spread = 0 | 1 (tier C: the members of a cluster dealt over the XCDs -- their exchange then goes through
 * memory instead of one XCD's L2; default: when that fits a quarter more clusters on the chip), cluster_timeout_s (tier C
 * watchdog per lattice column, default 30 s) and cluster_arrive_s (how long the first barrier of a launch waits for work-groups
 * of a cluster that have not been STARTED yet because something else holds their CUs, default 120 s: the members of a cluster
 * wait for each other, so a launch needs all of them resident; when either time runs out the launch is abandoned and the call
 * returns DNAS_E_DEVICE -- until then the waiting work-groups keep their CUs), sync_place = 0 | 1 (tier C, default 1: the words
 * the members of a cluster agree through are put where the device-scope round trip from the cluster's XCD measures shortest --
 * the memory channel matters: one read alone fills in 42 ms or 54 ms --, a few milliseconds when the model is made; 0: wherever
 * the allocation starts), tb_threads = threads per block of the
 * thread-per-read traceback (multiple of 64, at most 256, default 128) and tb_lanes = reads per wave there (1 .. 64, default 16:
 * the lanes of a wave stand on different states, and a step costs the wave the union of what they do), checkpoint = auto | always | never and
 * segment = columns (bounded-memory decode of reads whose lattice -- the reference's ViterbiMatrix::cell,
 * viterbi.h:48-50 -- does not fit the arena: segments of the lattice are filled from checkpoints and traced back one
 * after the other; results are bit-identical), traceback = thread, arena_fraction, plan_order = 0 | 1 | 2 and plan_slack = 0 .. 8
 * (the row program: states dealt depth first / breadth first / by longest-path level, there with that many eighths of the
 * room between a state's earliest and latest level used.  None given: the machine's tuning record decides -- shipped in
 * <library dir>/tune/, or found in the kernel cache; records = 0: the default program; autotune = 1: a tier-A machine
 * without a record is timed when its first model is created and the verdict kept in the kernel cache).  dnas_model_tier
 * names the program and the record that chose it.  A key that is absent falls back to the environment variable
 * DNAS_<KEY IN UPPER CASE>. */
int dnas_model_create_ex(const dnas_flat_model *fm, int device_id, size_t arena_bytes, const char *options,
                         dnas_model **out);
void dnas_model_destroy(dnas_model *model);

/*
 * The hot path: decodeFastSeqs' per-read loop (viterbi.cpp:312-318) for a batch.
 *   read_offsets[n_reads+1]  prefix offsets into bases
 *   bases[...]               one byte per nucleotide, values 0..3 (A,C,G,T)
 *   out_sym                  caller buffer; read i's decoded symbols go to
 *                            out_sym[out_offsets[i] .. out_offsets[i+1]) (no terminator)
 *   out_len[n_reads]         decoded length (0 for DNAS_READ_NO_PATH)
 *   out_loglike[n_reads]     ViterbiMatrix::loglike(), fp64 (viterbi.h:102)
 *   out_status[n_reads]      DNAS_READ_*
 * Host pointers; the call copies in, runs fill + traceback kernels, copies out, and
 * returns after the stream has drained.  A call with n_reads == 0 is a call too: it
 * resets the stats and leaves no lattice or event log of an earlier call readable.
 *
 * The slots.  out_offsets is the caller's: read i owns out_sym[out_offsets[i] .. out_offsets[i+1]) and nothing else, and
 * slots of any size, 0 included, may lie side by side.  A call writes no byte of out_sym outside the slots of its reads,
 * and a read writes none outside its own.  How long a decoded string gets is the machine's business, not the read's: a
 * walk decodes a symbol for every state it passes, with or without a base of the read.
 *   DNAS_READ_OK            the first out_len[i] bytes of the slot are the string; the rest of the slot is scratch
 *   DNAS_READ_OUT_OVERFLOW  the string is longer than the slot.  out_len[i] is 0, out_loglike[i] is the read's as ever, and
 *                           the whole slot is scratch, except that a slot of 8 bytes or more begins with the length the
 *                           string needs: a uint64, lowest byte first, whatever the slot's alignment (dnas_slot_needed
 *                           reads it).  Decoding that read again in a slot of that size gives the string.
 *   DNAS_READ_NO_PATH       out_len[i] is 0 and the slot is not written
 *   DNAS_READ_TRACEBACK_FAIL  out_len[i] is 0 and the slot is scratch
 * Callers inside this library that size the slots themselves (dnas_decode_fastseqs*, the command-line tool, the Python
 * front end's defaults) start from 4 L + 64 symbols for a read of L bases and decode the reads that overflow once more in
 * slots of the needed size; a caller that passes its own out_offsets gets the status and decides.
 */
int dnas_viterbi_batch(dnas_model *model, int64_t n_reads, const uint64_t *read_offsets, const uint8_t *bases,
                       char *out_sym, const uint64_t *out_offsets, uint32_t *out_len, double *out_loglike,
                       uint8_t *out_status);
/* The length a read with status DNAS_READ_OUT_OVERFLOW left in its slot (host memory, cap = the slot's size); 0 where the
 * slot is shorter than 8 bytes and holds none. */
uint64_t dnas_slot_needed(const char *slot, uint64_t cap);

/* Same, with bases and all outputs already resident in this GPU's HBM (device pointers);
 * read_offsets / out_offsets stay host arrays (they drive batching).  Asynchronous on the
 * model's own streams; dnas_model_sync waits.  The library does not know the caller's streams:
 * whatever produced d_bases (and any fill of the output buffers) must have completed before the
 * call, and the outputs may be read after dnas_model_sync.  n_reads == 0 as for dnas_viterbi_batch. */
int dnas_viterbi_batch_device(dnas_model *model, int64_t n_reads, const uint64_t *read_offsets,
                              const uint8_t *d_bases, char *d_out_sym, const uint64_t *out_offsets,
                              uint32_t *d_out_len, double *d_out_loglike, uint8_t *d_out_status);
int dnas_model_sync(dnas_model *model);

/*
 * Reads of unknown orientation.  A sequencer reports either strand of a molecule; the reference decodes a read only
 * as given, and a reverse-complemented read decodes to a confident-looking wrong string (its log-likelihood is finite,
 * tens of nats below the right orientation's).  strand_mode says which orientation of every read is decoded:
 *   DNAS_STRAND_FORWARD  the read as given: dnas_viterbi_batch[_device] itself, out_strand filled with zeros;
 *   DNAS_STRAND_REVERSE  its reverse complement (3 - base, order reversed): the result is that of
 *                        dnas_viterbi_batch on the reverse-complemented reads, out_strand filled with ones;
 *   DNAS_STRAND_BOTH     per read, F = the result for the read and R = the result for its reverse complement; the
 *                        call returns R with out_strand = 1 iff R's log-likelihood is strictly larger (fp64 compare),
 *                        else F with out_strand = 0.  Ties -- every reverse-palindromic read, the empty read -- go to
 *                        the forward strand; two -inf give DNAS_READ_NO_PATH, strand 0, an empty string.  Symbols,
 *                        log-likelihood and status are bit-identical to what dnas_viterbi_batch returns for the
 *                        winning orientation given as a read of its own.  Both lattices are filled (the fill's cost
 *                        doubles); only the winner is traced back.
 * Pointer conventions as dnas_viterbi_batch / dnas_viterbi_batch_device; out_strand is uint8_t[n_reads] (a device
 * pointer in the _device form).  Event log (dnas_model_set_event_log): the events of a read that was decoded from its
 * reverse complement are those of that decode, positions counted along the reverse-complemented read;
 * dnas_model_read_events takes the caller's read index in every mode.  dnas_model_read_lattice after a
 * DNAS_STRAND_BOTH call returns DNAS_E_UNSUPPORTED.  Bounded-memory decode (option checkpoint=): the first pass runs for
 * both orientations, the second fill of every segment and the traceback for the winners only;
 * dnas_batch_stats.checkpointed_reads and .columns of a DNAS_STRAND_BOTH call count orientations (2 per read).
 */
#define DNAS_STRAND_FORWARD 0
#define DNAS_STRAND_REVERSE 1
#define DNAS_STRAND_BOTH 2
int dnas_viterbi_batch_strands(dnas_model *model, int64_t n_reads, const uint64_t *read_offsets, const uint8_t *bases,
                               int strand_mode, char *out_sym, const uint64_t *out_offsets, uint32_t *out_len,
                               double *out_loglike, uint8_t *out_status, uint8_t *out_strand);
int dnas_viterbi_batch_strands_device(dnas_model *model, int64_t n_reads, const uint64_t *read_offsets,
                                      const uint8_t *d_bases, int strand_mode, char *d_out_sym,
                                      const uint64_t *out_offsets, uint32_t *d_out_len, double *d_out_loglike,
                                      uint8_t *d_out_status, uint8_t *d_out_strand);
/* Host helper, no GPU: out[i] = 3 - bases[n - 1 - i] (out must not overlap bases); a code above 3: DNAS_E_BAD_BASE. */
int dnas_reverse_complement(const uint8_t *bases, size_t n, uint8_t *out);
/* What the last call did about strands (after dnas_model_sync); all zero after a forward call.  tracebacks = reads a
 * traceback kernel was launched over; fill_columns = sum of L + 1 over every lattice filled (the first pass of the
 * bounded-memory decode); pass2_columns = sum of L + 1 over the reads its second pass fills again and traces back.
 * reverse_won, ties (equal log-likelihoods, the pairs of -inf among them) and both_no_path (both -inf) are counted by
 * the kernel that picks the strand: zero in mode DNAS_STRAND_REVERSE, where nothing is picked. */
typedef struct dnas_strand_stats {
  int64_t reads, reverse_won, ties, both_no_path, tracebacks, fill_columns, pass2_columns;
} dnas_strand_stats;
int dnas_model_last_strand_stats(const dnas_model *model, dnas_strand_stats *out);

/* Which fill kernel serves this model: "tier A: <shape>" (register/LDS-resident kernel, JIT-specialised
 * for the machine; "...W8 ... 2 work-groups per CU": a small row program compiled so that two reads share a CU), "tier C: <n>
 * work-groups per read, ..." (the same kernel on a cluster of work-groups) or "tier B: <reason>" (general global-memory
 * kernel); behind it the tuning record that chose the row program.  DNAS_TIER=B forces tier B. */
const char *dnas_model_tier(const dnas_model *model);
/* Keep the traceback's event log (see dnas_decode_fastseqs_ex) for the following calls; dnas_model_read_events
 * returns the events of read `read_index` of the last call (out may be NULL to ask for the count), and refuses
 * when that call ran without the log or had no reads.  The log is the model's own buffer and holds every event of every
 * read: a call whose first sizing of it (3 L + 64 events a read) proves too small runs a second time with the sizes the
 * first run counted, so with the log on a call costs up to twice its time and a _device call has finished when it returns.
 * *n_events is the number of events the traceback met, and all of them are there to be read; should a log ever hold fewer,
 * dnas_model_read_events fails with DNAS_E_DEVICE rather than hand out a short list. */
int dnas_model_set_event_log(dnas_model *model, int on);
int dnas_model_read_events(dnas_model *model, int64_t read_index, uint64_t *out, int64_t cap, int64_t *n_events);
/* Specialise + compile the tier-A kernel for a machine ahead of time (no GPU needed). */
int dnas_tiera_precompile(const dnas_flat_model *fm, char *note, size_t note_cap);

/* Tier C: the same kernel run by a cluster of `members` work-groups per read (machines beyond one CU).
 * dnas_tierc_precompile compiles it ahead of time (members = 0: the smallest cluster that fits; no GPU needed).
 * dnas_tierc_plan is an analysis / test aid: the tables exactly as the kernel receives them.  info[8] =
 * {members, rows, threads, entries per member, S stripes, inbox rows, proxies, 0}; the other outputs may be NULL:
 * row_shapes[rows][6] = {entries, S stripe, kind, class, full, entries into another member's inbox: 0 none /
 * 1 all / 2 mixed}, entries[members][entries][threads], meta[members][rows][threads], member_of[n_states],
 * lds_index[n_states] = row*threads + lane inside the member, lattice_slot[n_states],
 * fold[members][inbox rows][threads] = the LDS cells behind every inbox cell (one cell per edge between two members).
 * dnas_tierc_plan_proxies: member and lds_index of the plan's proxies (places that hold no state of the machine: they
 * combine the null edges of one member into one state of another and forward the maximum over ONE edge), info[6] of them.
 * members = 1 describes the tier-A plan.  dnas_model_cluster_census: clusters that ran in the last call and how
 * many of them had members on more than one XCD (placement is a speed matter only). */
int dnas_tierc_precompile(const dnas_flat_model *fm, int32_t members, char *note, size_t note_cap);
int dnas_tierc_plan(const dnas_flat_model *fm, int32_t members, int32_t *info, int32_t *row_shapes, uint32_t *entries,
                    size_t entries_cap, uint32_t *meta, int32_t *member_of, int32_t *lds_index, int32_t *lattice_slot,
                    uint32_t *fold);
int dnas_tierc_plan_proxies(const dnas_flat_model *fm, int32_t members, int32_t *proxy_member, int32_t *proxy_lds_index, size_t cap);
int dnas_model_cluster_census(dnas_model *model, int32_t *clusters, int32_t *split);
/* The file name of a machine's row-program tuning record -- members = 1: as tier A (threads = 0: 1024); members = 0 or >= 2: as
 * tier C with the smallest / that cluster (threads as given to the model, 0 = the planner's choice) --: "tune_<hash>.txt", looked
 * for in the kernel cache and in <library dir>/tune/.  The name hashes the machine's graph, the work-group shape and the
 * planner version.  A record starts with "order=<0|1|2> slack=<0..8> kernel=<hash>" (options plan_order, plan_slack; the
 * hash of the kernel source the verdict was measured with, see dnas_kernel_source_hash). */
int dnas_tune_record_name(const dnas_flat_model *fm, int32_t members, int32_t threads, char *out, size_t cap);
/* The hash of the fill kernel's source as this library carries it, 16 hex digits: what the tuning records name as
 * "kernel=".  A record measured with another source is still followed; dnas_model_tier then says "stale". */
int dnas_kernel_source_hash(char *out, size_t cap);

/* Analysis / test aid: where tier A puts each state (lds_index = row*threads + lane; lattice_slot = its
 * position inside a lattice row).  No GPU needed.  DNAS_E_UNSUPPORTED when the machine does not fit tier A. */
int dnas_tiera_plan_slots(const dnas_flat_model *fm, int32_t *lds_index, int32_t *lattice_slot, int32_t *threads,
                          int32_t *rows);

/* Analysis / test aid: the tier-A tables exactly as the fill kernel receives them (layout:
 * dnastore_amd/csrc/viterbi_tiera.hip).  row_shapes[rows][2] = {out-edge entries, S stripe or -1};
 * entries[n_entries][threads]; meta[rows][threads].  Any output may be NULL. */
int dnas_tiera_plan_tables(const dnas_flat_model *fm, int32_t *row_shapes, uint32_t *entries, size_t entries_cap,
                           uint32_t *meta, int32_t *n_entries, int32_t *n_s_rows);

/* Diagnostic: 8 words of the kernel's rounds/stamp buffer (word 0 = total rounds; words 1-5 are filled only by
 * a -DDNAS_STAMP diagnostic build selected with DNAS_TIERA_DEFS). */
int dnas_model_debug_words(dnas_model *model, unsigned long long *out8);

/* Device-time accounting of the last batch call (HIP events on the model's streams); all zero after a call
 * with no reads. */
typedef struct dnas_batch_stats {
  double fill_ms, traceback_ms;   /* fill_ms: the time during which at least one fill launch of the call ran -- the union of the
                                     launches' intervals; the sum of their durations where they do not overlap (dnas_model_last_arena_slices < 3).
                                     traceback_ms: summed kernel durations (the tracebacks of a call are serial) */
  int64_t fill_launches, columns; /* launches; sum over reads of L+1  */
  int64_t lattice_bytes;          /* 8*(D+2)*N*columns (algorithmic)  */
  int64_t rounds;                 /* relaxation rounds, summed        */
  int64_t checkpointed_reads;     /* reads decoded in segments (bounded-memory decode: option checkpoint=) */
} dnas_batch_stats;
int dnas_model_last_stats(const dnas_model *model, dnas_batch_stats *out);
/* How many batches' lattices the last batch call kept side by side: 1, 2 (arena halves in turn) or 3 (the ring of option
 * fill_overlap); 0 after a call with no reads.  (Not a member of dnas_batch_stats: that struct keeps its layout.) */
int dnas_model_last_arena_slices(const dnas_model *model, int64_t *out);

/* Copy one read's lattice out of the arena after a single-read batch (testing aid):
 * layout [pos][lane][n_states], lanes S, D, T1..TD.  `slot` is a read of the last call: after a call
 * with no reads there is none. */
int dnas_model_read_lattice(dnas_model *model, int64_t slot, int64_t len, double *out);

/* ---- forward-backward path ------------------------------------------------------------ */

/*
 * expectedCounts(params, db, ll, strict) (reference src/fwdback.cpp:190-209): the E-step of the
 * mutator pair-HMM over a database of (original, read) alignment pairs, one GPU thread per pair.
 * Pairs are concatenated: pair i is in_seqs[in_off[i]..in_off[i+1]) / out_seqs[...] (bases 0..3)
 * with the guide alignment given per sequence position as the cumulative match count at that
 * position's alignment column (GuideAlignmentEnvelope, alignpath.h:35-54):
 *   cm_in[cm_in_off[i] + ip],  ip = 0..inLen;   cm_out[cm_out_off[i] + op],  op = 0..outLen.
 * out_counts[21 + n_len]: nDelOpen, nTanDup, nNoGap, nDelExtend, nDelEnd, nSub[4][4], nLen[]
 * (MutatorCounts, mutator.h:43-50); *out_ll = sum of forward log-likelihoods; out_pair_ll
 * (optional, n_pairs) the per-pair values.  Host pointers.  device_id = -1: every GPU of the node (see dnas_fb_create).
 */
int dnas_fwdback_estep(const dnas_mutator_params *params, int strict, int64_t n_pairs, const int8_t *in_seqs,
                       const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const int32_t *cm_in,
                       const int64_t *cm_in_off, const int32_t *cm_out, const int64_t *cm_out_off, int device_id,
                       double *out_counts, double *out_ll, double *out_pair_ll);

/* The same E-step behind a persistent handle: the log-sum-exp table (per device) and the database (per load) go to
 * the GPU once; dnas_fb_estep then runs on the handle's own stream with buffers it keeps -- the EM loop calls it up
 * to 100 times.  Pairs whose envelope rows are at most 32 cells wide (and n_len <= 8) are served by the wavefront
 * kernels (a group of 8, 16 or 32 lanes per pair, neighbours by lane shuffle); the rest by the streaming kernel.  dnas_fwdback_estep and
 * dnas_baum_welch are built on this.
 *
 * dnas_fb_create(-1, ...): every GPU of the node (DNAS_FAKE_DEVICES=n, read when the handle is made: n devices d % visible GPUs).
 * The handle holds one handle as above per device; dnas_fb_load_pairs checks the offsets of the whole database (messages name the
 * caller's pair index), deals the pairs over the devices by inLen + outLen (longest first, snake order) and loads every shard, one
 * host thread per device; a device may get no pairs.  A failure on a device returns the code a one-device handle would, the
 * message prefixed with "device <d>: ", and leaves the handle without a database.  dnas_fb_estep runs every device's E-step at
 * once (one host thread per device) and adds the devices' counts and log-likelihoods on the host in device order; out_pair_ll
 * is in the caller's order.  dnas_fb_last_stats: the pair counts, out_nt and lse_ops summed over the devices, kernel_ms the largest.
 * Results with W > 1 devices: per-pair log-likelihoods are bit-identical to a one-device handle; counts and the summed
 * log-likelihood equal a one-device handle up to the order of summation (relative 1e-12); results are bit-identical from call
 * to call for a fixed W.  With W = 1 they are bit-identical to device_id = 0.  Other negative device_ids: DNAS_E_INVALID. */
typedef struct dnas_fb dnas_fb;
typedef struct dnas_fb_stats {
  double kernel_ms;                 /* E-step kernels of the last call (HIP events on the handle's stream) */
  int64_t pairs_onchip, pairs_streaming;
  int64_t lse_ops;                  /* log_sum_exp evaluations of the on-chip kernel (counted in the kernel) */
  int64_t out_nt;                   /* sum of the read (output) lengths */
  int64_t pairs_narrow;             /* ... of pairs_onchip: served with half as many lanes as the row capacity (alignments that run down a diagonal) */
} dnas_fb_stats;
int dnas_fb_create(int device_id, dnas_fb **out);
int dnas_fb_load_pairs(dnas_fb *h, int64_t n_pairs, const int8_t *in_seqs, const int64_t *in_off, const int8_t *out_seqs,
                       const int64_t *out_off, const int32_t *cm_in, const int64_t *cm_in_off, const int32_t *cm_out,
                       const int64_t *cm_out_off);
int dnas_fb_estep(dnas_fb *h, const dnas_mutator_params *params, int strict, double *out_counts, double *out_ll,
                  double *out_pair_ll);
int dnas_fb_last_stats(const dnas_fb *h, dnas_fb_stats *out);
int dnas_fb_devices(const dnas_fb *h);   /* how many devices share the handle (1 for a one-device handle) */
void dnas_fb_destroy(dnas_fb *h);

/* baumWelchParams(init, Laplace prior, db, strict) (fwdback.cpp:211-230, dnastore.cpp:135-140):
 * EM on the host around the GPU E-step; at most 100 iterations, stops when the relative gain
 * of log(likelihood * prior) drops below 1e-3.  One handle for the whole fit; device_id = -1: every GPU of the node
 * (dnas_fb_create). */
int dnas_baum_welch(const dnas_mutator_params *init, int strict, int64_t n_pairs, const int8_t *in_seqs,
                    const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const int32_t *cm_in,
                    const int64_t *cm_in_off, const int32_t *cm_out, const int64_t *cm_out_off, int device_id,
                    dnas_mutator_params *out, int32_t *out_iterations);

/* Stockholm database of two-row (original, read) alignments, readStockholmDatabase + Alignment +
 * GuideAlignmentEnvelope (stockholm.cpp:154-167, alignpath.cpp:189-204,237-265), flattened into the
 * arrays dnas_fwdback_estep takes. */
typedef struct dnas_pairs dnas_pairs;
typedef struct dnas_pairs_view {
  int64_t n_pairs;
  const int8_t *in_seqs;  const int64_t *in_off;
  const int8_t *out_seqs; const int64_t *out_off;
  const int32_t *cm_in;   const int64_t *cm_in_off;
  const int32_t *cm_out;  const int64_t *cm_out_off;
} dnas_pairs_view;
int dnas_stockholm_read(const char *path, dnas_pairs **out);
const dnas_pairs_view *dnas_pairs_get(const dnas_pairs *p);
void dnas_pairs_free(dnas_pairs *p);

/* ---- aligning unaligned (original, read) pairs ------------------------------------------ */

/*
 * The database above needs a guide alignment per pair; a sequencing run has none.  dnas_align_pairs finds it with the model's
 * own likelihood as the objective: the most probable path of the mutator pair HMM between the two sequences (the max-plus
 * twin of the Forward matrix of the E-step), traced back to a gapped pair.  The reference has no counterpart.
 *
 * The model.  in[0..I) and out[0..O) are base codes 0..3, P = n_len, the scores are MutatorScores (dnas_mutator_scores).
 * Cell (ip, op), 0 <= ip <= I, 0 <= op <= O, has lanes S, D and T_k for k < min(ip, P); everything starts at -inf except
 * S(0,0) = 0; every sum is formed left to right in fp64:
 *   D(ip,op)   = best of  [d0] S(ip-1,op) + delOpen        [d1] D(ip-1,op) + delExtend                  (ip > 0)
 *   S(ip,op)   = best of  [s0] S(ip-1,op-1) + noGap + sub[in[ip-1]][out[op-1]]                          (ip > 0, op > 0)
 *                         [s1] T_0(ip,op-1) + sub[in[ip-1]][out[op-1]]                                  (ip > 0, op > 0, P > 0)
 *                         [s2] D(ip,op) + delEnd
 *   T_k(ip,op) = best of  [t0] T_{k+1}(ip,op-1) + sub[in[ip-2-k]][out[op-1]]                            (op > 0, k+1 < min(ip,P))
 *                         [t1] S(ip,op) + tanDup + len[k]
 * "best of" takes the candidates in the order listed; the first strictly greater one wins.  With d = op - ip a cell is
 * inside the band iff min(0, O-I) - band <= d <= max(0, O-I) + band; a candidate that reads a cell outside it is -inf;
 * band = DNAS_ALIGN_FULL: every cell.  The score is S(I,O); the traceback goes from (I,O,S) along the recorded choices to
 * (0,0,S) and yields the columns in alignment order: s0 a match column, d0 / d1 a deletion column (input base over a gap),
 * s1 / t0 a duplication column (a gap over the output base).
 *
 * Pairs are concatenated as for dnas_fwdback_estep: pair i is in_seqs[in_off[i]..in_off[i+1]) / out_seqs[out_off[i]..).
 *   out_ops            one byte per alignment column, kind | n << 2: kind 0 match, 1 deletion, 2 duplication; n is non-zero only
 *                      on the first column of an event -- 1 where a deletion opens (d0), the duplication's length k + 1 where
 *                      one opens -- so the path is kept whole: two duplications of length 1 differ from one of length 2, a
 *                      deletion that ends and opens again (D -> S -> D) from one that is extended.  Pair i's columns go to
 *                      out_ops[ops_off[i] ..); the slot ops_off[i+1] - ops_off[i] must hold inLen + outLen bytes
 *                      (DNAS_E_INVALID otherwise)
 *   out_n_ops[n_pairs] columns written (0 unless the status is DNAS_ALIGN_OK)
 *   out_score[n_pairs] S(I,O); -inf with DNAS_ALIGN_NO_PATH (I = 0 and O > 0 is an example), NaN with DNAS_ALIGN_TOO_LARGE
 *   out_status[n_pairs] DNAS_ALIGN_*
 *   out_stats          may be NULL
 * Host pointers.  n_len > 13: DNAS_E_UNSUPPORTED (a cell's choices are P + 3 bits of a 16-bit word, the limit the event log
 * has); a base code outside 0..3: DNAS_E_BAD_BASE; n_pairs = 0 is a valid call.  The GPU keeps one 16-bit choice word per
 * cell of the band (and of the skew of its wavefront) in an arena: arena_bytes = 0 takes a fraction of the free HBM, any
 * other value that many bytes, and the call runs in as many batches as the arena needs; a pair whose record alone exceeds
 * the arena gets DNAS_ALIGN_TOO_LARGE and leaves the other pairs of the call alone.  device_id = -1: the pairs are dealt over
 * the GPUs of the node (DNAS_FAKE_DEVICES as for dnas_fb_create) by (I + 1) x band width, costliest first in snake order,
 * one host thread per device; results come back in the caller's order.  Score, ops and status are bit-identical to
 * dnas_align_pairs_host whatever the device count and the batching.  DNAS_ALIGN_BLOCKS=n (testing aid) caps the fill's grid at
 * n work-groups of four waves, so that a short list already makes every wave walk several pairs.
 */
#define DNAS_ALIGN_FULL (-1)
#define DNAS_ALIGN_OK 0
#define DNAS_ALIGN_NO_PATH 1
#define DNAS_ALIGN_TOO_LARGE 2
#define DNAS_ALIGN_TRACEBACK_FAIL 3   /* the recorded choices do not lead back to (0,0): a defect, never a property of the input */
typedef struct dnas_align_stats {
  double fill_ms, traceback_ms;   /* summed kernel durations (HIP events); with several devices the slowest device's */
  int64_t cells;                  /* cells inside the band, all pairs */
  int64_t batches;                /* fill launches (summed over the devices) */
  int64_t pairs_too_large;
} dnas_align_stats;
int dnas_align_pairs(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                     const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, int device_id, size_t arena_bytes,
                     uint8_t *out_ops, const uint64_t *ops_off, uint32_t *out_n_ops, double *out_score, uint8_t *out_status,
                     dnas_align_stats *out_stats);
/* The same on the host, no GPU needed: one thread, the matrices of the whole band kept (csrc/host/pairalign.cpp).  It is the
 * statement of the model the kernels are held to, and the CPU baseline.  Never DNAS_ALIGN_TOO_LARGE. */
int dnas_align_pairs_host(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                          const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, uint8_t *out_ops,
                          const uint64_t *ops_off, uint32_t *out_n_ops, double *out_score, uint8_t *out_status);
/* MutatorScores of the parameters (mutator.cpp:56-75), the logarithms exactly as every kernel here receives them:
 * out[21 + n_len] = delOpen, tanDup, noGap, delExtend, delEnd, sub[16] (sub[base*4+observed]), len[]. */
int dnas_mutator_scores(const dnas_mutator_params *params, double *out);
/* One pair's op bytes spelled out (host helper); any output may be NULL.  row_in / row_out: the two gapped rows, upper case
 * with '-', n_ops characters and a NUL; cm_in[in_len + 1] / cm_out[out_len + 1]: the guide arrays dnas_stockholm_read derives
 * from those rows (what dnas_fwdback_estep takes); counts[21 + n_len]: the moves of the path in MutatorCounts order (per match
 * column nNoGap and nSub, per duplication column nSub against the copied input base, per duplication nTanDup and nLen[k], per
 * deletion nDelOpen, nDelExtend per further column and nDelEnd): the sum of counts x scores is the score.  Ops that are not a
 * path of the model over these sequences: DNAS_E_INVALID. */
int dnas_alignment_expand(int32_t n_len, const int8_t *in, int64_t in_len, const int8_t *out, int64_t out_len,
                          const uint8_t *ops, int64_t n_ops, char *row_in, char *row_out, int32_t *cm_in, int32_t *cm_out,
                          double *counts);
/* The Stockholm database of n_pairs gapped pairs: per pair "# STOCKHOLM 1.0", two "name row" lines and "//", malloc'd and
 * NUL-terminated (dnas_free).  dnas_stockholm_read gives back the arrays the rows stand for.  The reader merges rows of equal
 * names, so a read named like its original is written with the suffix "/read".  Names are single words; rows without
 * columns cannot be written (DNAS_E_INVALID). */
int dnas_stockholm_write(int64_t n_pairs, const char *const *names_in, const char *const *names_out,
                         const char *const *rows_in, const char *const *rows_out, char **text, size_t *len);

/* ---- the marginal likelihood of a pair: the forward score --------------------------------- */

/*
 * S(I,O) of dnas_align_pairs is the score of the single most probable alignment: a ranking score, not the likelihood of the
 * read given the original.  dnas_pair_likelihoods returns log P(read | original), summed over every alignment inside the band:
 * the same lattice, band and start, with "best of" replaced by log-sum-exp.
 *   D(ip,op)   = lse( S(ip-1,op) + delOpen ,  D(ip-1,op) + delExtend )                                   (ip > 0)
 *   S(ip,op)   = lse( lse( S(ip-1,op-1) + noGap + sub[in[ip-1]][out[op-1]] ,
 *                          T_0(ip,op-1) + sub[in[ip-1]][out[op-1]] ) ,
 *                     D(ip,op) + delEnd )
 *   T_k(ip,op) = lse( T_{k+1}(ip,op-1) + sub[in[ip-2-k]][out[op-1]] ,  S(ip,op) + tanDup + len[k] )      (k < min(ip,P))
 * S(0,0) = 0; a term whose condition does not hold (those of dnas_align_pairs) or whose cell is outside the band is -inf; sums
 * inside a term are formed left to right in fp64, the lse calls nest as written.  lse(a, b) = max + f(|a - b|) with f the
 * reference's table of log(1 + exp(-x)), the one the E-step uses: 100 001 entries 1e-4 apart, interpolated linearly, 0 from
 * x = 10 on.  lse(-inf, -inf) = -inf and lse(x, -inf) = x exactly.  Against an exact log-sum-exp the table drops at most e^-10
 * and overshoots by less than 1e-9 per call, so with n = 6 (I + O + 1):  exact - n (e^-10 + 1e-9) <= result <= exact + n 1e-9.
 *
 * Pairs are concatenated as for dnas_align_pairs; out_rev[n_pairs], or NULL for all zeros: 1 = the read is scored as its
 * reverse complement, read in place.
 *   out_ll[n_pairs]   S(I,O); -inf when no path lies inside the band
 *   out_stats         may be NULL
 * Checks as for dnas_align_pairs (n_len > 13: DNAS_E_UNSUPPORTED, a base code outside 0..3: DNAS_E_BAD_BASE, offsets);
 * n_pairs = 0 is a valid call; band = DNAS_ALIGN_FULL (-1): every cell.  device_id = -1: the pairs are dealt over the GPUs of
 * the node as dnas_align_pairs deals them, results come back in the caller's order.  A wave owns a pair and walks the
 * wavefront of dnas_align_pairs with the sum-product cell; launch plan, chunk loop and device fan-out are those of the other
 * score kernels.  Testing aids: DNAS_FORWARD_CHUNK=n caps a launch at n pairs, DNAS_ALIGN_BLOCKS=n the grid.
 *
 * dnas_pair_likelihoods_host is the statement (csrc/host/pairforward.cpp): one thread, rolling rows, no GPU;
 * dnas_pair_likelihoods is bit-identical to it with exact_lse = 0 whatever the device count, the grid and the chunking.
 * exact_lse = 1 replaces the table by max + log1p(exp(-|a - b|)) of the host libm (host only).
 */
#define DNAS_SCORE_VITERBI 0
#define DNAS_SCORE_FORWARD 1
typedef struct dnas_forward_stats {
  double score_ms;   /* summed kernel durations (HIP events); with several devices the slowest device's */
  int64_t items;     /* pairs scored */
  int64_t cells;     /* cells inside the band, all pairs */
  int64_t chunks;    /* score-kernel launches (summed over the devices) */
} dnas_forward_stats;
int dnas_pair_likelihoods(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                          const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                          int device_id, double *out_ll, dnas_forward_stats *out_stats);
int dnas_pair_likelihoods_host(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                               const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                               int exact_lse, double *out_ll);

/* ---- posterior move counts over the whole band: the backward pass, Baum-Welch on unaligned pairs ---- */

/*
 * dnas_fwdback_estep counts the moves of the model inside the envelope of a guide alignment.  dnas_pair_counts counts them over
 * every alignment inside the band of dnas_pair_likelihoods, with no guide: the lattice, band, start, scores and lse are those
 * of the forward score above, F_S, F_D and F_Tk its values bit for bit, Z = F_S(I,O).  With ip, op the bases consumed:
 *   B_S(I,O)    = 0
 *   B_Tk(ip,op) = sub[in[ip-1-k]][out[op]] + (k > 0 ? B_T{k-1}(ip,op+1) : B_S(ip,op+1))                 (k < min(ip,P), op < O)
 *   B_S(ip,op)  = tree( (noGap + sub[in[ip]][out[op]]) + B_S(ip+1,op+1) ,  delOpen + B_D(ip+1,op) ,
 *                       (tanDup + len[0]) + B_T0(ip,op) , ... , (tanDup + len[n-1]) + B_T{n-1}(ip,op) )   n = min(ip,P)
 *   B_D(ip,op)  = lse( delExtend + B_D(ip+1,op) ,  delEnd + B_S(ip,op) )
 * A term that reads a cell outside the band or the matrix is -inf; inside a cell the order is T_k, S, D.  tree(v_0 .. v_{m-1})
 * combines neighbours level by level, v_i <- lse(v_2i, v_2i+1), an odd last element carried up unchanged, until one is left:
 * depth ceil(log2(n + 2)), and P = 0 is the tree of the first two terms.  B_S(0,0) is the backward likelihood.
 *
 * The posterior of a move n -> n' of weight w is exp(F(n) + w + B(n') - Z), the exponent summed left to right (w's parts in
 * the order written above for the forward score: noGap + sub, tanDup + len[k]), and it is added to each of the move's counts:
 *   S(ip,op) -> S(ip+1,op+1): nNoGap, nSub[in[ip]][out[op]]     S(ip,op) -> D(ip+1,op): nDelOpen
 *   S(ip,op) -> T_k(ip,op): nTanDup, nLen[k]                     D(ip,op) -> D(ip+1,op): nDelExtend     D(ip,op) -> S(ip,op): nDelEnd
 *   T_k(ip,op) -> T_{k-1}(ip,op+1), or S(ip,op+1) for k = 0: nSub[in[ip-1-k]][out[op]]
 * Counts are laid out as MutatorCounts, [21 + n_len]: nDelOpen, nTanDup, nNoGap, nDelExtend, nDelEnd, nSub[16], nLen[].  The
 * host statement adds them in cell order (rows last to first, columns right to left).  The kernel adds per lane in step order
 * (a lane owns row 64 s + l; stripes last to first, steps right to left; inside a cell match, delOpen, the duplications by k,
 * delExtend, delEnd, the T_k emissions by k), then sums the 64 lanes in a fixed tree: lane l takes lane l + 32, then l + 16,
 * 8, 4, 2, 1.  The two differ by the rounding of a sum of non-negative terms and by the device's exp.
 *
 *   out_counts[21 + n_len], out_ll    sums over the pairs with status OK, formed on the host from the per-pair values in pair
 *                                     order: they do not depend on the grid, the chunking or the device count
 *   out_pair_counts[n_pairs x (21 + n_len)]  may be NULL
 *   out_pair_ll[n_pairs]              Z, the bits of dnas_pair_likelihoods; NaN with DNAS_COUNTS_TOO_LARGE
 *   out_pair_ll_backward[n_pairs]     B_S(0,0), may be NULL (a testing aid; -inf with NO_PATH, NaN with TOO_LARGE)
 *   out_status[n_pairs]               DNAS_COUNTS_OK | DNAS_COUNTS_NO_PATH (Z = -inf: counts zero, left out of every sum) |
 *                                     DNAS_COUNTS_TOO_LARGE (counts zero, left out of every sum)
 * Checks as for dnas_pair_likelihoods; device_id = -1 as for dnas_align_pairs.  A wave owns a pair: pass 1 is the forward
 * kernel's cell with every finished S, D and T_k parked in the wave's scratch in HBM, n_len + 2 planes of one double per slot of
 * the wavefront of the largest pair the wave may meet; pass 2 walks the wavefront backwards and meets each parked cell in the
 * lane that parked it.  The grid is cut so that the scratch of all its waves fits arena_bytes (0: what the call needs, up to
 * half of the free HBM); a pair whose scratch alone exceeds the arena gets DNAS_COUNTS_TOO_LARGE and leaves the others alone.
 * Testing aids: DNAS_COUNTS_CHUNK=n pairs per launch, DNAS_ALIGN_BLOCKS=n the grid.
 *
 * dnas_pair_counts_host is the statement (csrc/host/paircounts.cpp), one thread, never TOO_LARGE.  With exact_lse = 0 its
 * out_pair_ll and out_pair_ll_backward are bit-identical to the GPU's.
 */
#define DNAS_COUNTS_OK 0
#define DNAS_COUNTS_NO_PATH 1
#define DNAS_COUNTS_TOO_LARGE 2
typedef struct dnas_counts_stats {
  double kernel_ms;          /* summed kernel durations (HIP events; both passes share a launch); several devices: the slowest's */
  int64_t cells;             /* cells inside the band, all pairs that were run */
  int64_t chunks;            /* kernel launches (summed over the devices) */
  int64_t scratch_bytes;     /* parked forward cells: bytes allocated (summed over the devices) */
  int64_t pairs_too_large;
  int64_t waves;             /* waves of the grid the arena allowed (summed over the devices) */
} dnas_counts_stats;
int dnas_pair_counts(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                     const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev, int device_id,
                     size_t arena_bytes, double *out_counts, double *out_ll, double *out_pair_counts, double *out_pair_ll,
                     double *out_pair_ll_backward, uint8_t *out_status, dnas_counts_stats *out_stats);
int dnas_pair_counts_host(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                          const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                          int exact_lse, double *out_counts, double *out_ll, double *out_pair_counts, double *out_pair_ll,
                          double *out_pair_ll_backward, uint8_t *out_status);

/*
 * dnas_pair_counts sums each move's posterior over the whole matrix; dnas_pair_profiles keeps where along the original it fell.
 * Lattice, band, scores, lse, F, B and Z are those of dnas_pair_counts unchanged.  For a pair with original in[0..I) and
 * oriented read out[0..O), every row r = 0..I has W = 6 + n_len planes, each the sum over the columns op of row r inside the
 * band, in descending op, of the posterior exp(F + w + B' - Z) dnas_pair_counts forms for these moves out of cell (r, op):
 *   DNAS_PROFILE_MATCH + y       S(r,op) -> S(r+1,op+1) with out[op] == y (r < I, op < O): in[r] was read, as base y
 *   DNAS_PROFILE_DEL_OPEN        S(r,op) -> D(r+1,op): in[r] deleted, opening a gap
 *   DNAS_PROFILE_DEL_EXTEND      D(r,op) -> D(r+1,op): in[r] deleted, extending one
 *   DNAS_PROFILE_DUP + k         S(r,op) -> T_k(r,op), k < n_len: a duplication of k + 1 bases inserted in front of in[r]
 *                                (after in[I-1] for r = I)
 * D -> S and the T_k emissions consume no base of the original and are not profiled; row I holds only the duplication planes.
 * Every path consumes each in[r] exactly once: for r < I the four match planes and the two deletion planes sum to 1, and the
 * sums over r are nNoGap, nDelOpen, nDelExtend and nLen[k] of dnas_pair_counts.
 *
 *   out_pair_profiles   may be NULL; pair i's block starts at W (in_off[i] + i) doubles and is plane-major: plane j of row r at
 *                       block + j (I + 1) + r.  NO_PATH and TOO_LARGE pairs have all-zero blocks and are left out of every sum
 *   out_profile[(5 + n_len) x n_positions], out_coverage[n_positions]   the aggregate, formed on the host from the per-pair
 *                       blocks in pair order over the OK pairs: bit-identical whatever the grid, chunking and device count.
 *                       Row r of a pair adds to position p = r (anchor DNAS_PROFILE_FROM_START, from the 5' end) or p = I - r
 *                       (DNAS_PROFILE_FROM_END, from the 3' end); rows with p >= n_positions are dropped; coverage[p] counts
 *                       the OK pairs with a row at p.  An aggregate over different originals cannot keep absolute bases, so the
 *                       match planes are folded relative to in[r]: DNAS_PROFILE_SAME (y == in[r]), DNAS_PROFILE_TRANSITION
 *                       (y == in[r] ^ 2 in the ACGT coding), DNAS_PROFILE_TRANSVERSION (the other two, lower y first), then
 *                       DNAS_PROFILE_SUM_DEL_OPEN, DNAS_PROFILE_SUM_DEL_EXTEND, DNAS_PROFILE_SUM_DUP + k.  Both may be NULL
 *                       with n_positions = 0
 *   out_pair_ll[n_pairs]   Z, the bits of dnas_pair_likelihoods; NaN with DNAS_COUNTS_TOO_LARGE
 *   out_status, out_stats, checks, device_id, arena_bytes, testing aids   as dnas_pair_counts
 * The kernel (csrc/pair_profile_kernels.hip) is the two passes of dnas_pair_counts with the backward pass's accumulators stored
 * per (stripe, lane) -- a lane stands on one row for a whole stripe -- instead of summed over the lanes: each value is one
 * lane's sum in step order, the order of the host statement, so it differs from dnas_pair_profiles_host (csrc/host/
 * paircounts.cpp, one thread, never TOO_LARGE) with exact_lse = 0 by the device's exp only.
 */
#define DNAS_PROFILE_MATCH 0
#define DNAS_PROFILE_DEL_OPEN 4
#define DNAS_PROFILE_DEL_EXTEND 5
#define DNAS_PROFILE_DUP 6
#define DNAS_PROFILE_SAME 0
#define DNAS_PROFILE_TRANSITION 1
#define DNAS_PROFILE_TRANSVERSION 2
#define DNAS_PROFILE_SUM_DEL_OPEN 3
#define DNAS_PROFILE_SUM_DEL_EXTEND 4
#define DNAS_PROFILE_SUM_DUP 5
#define DNAS_PROFILE_FROM_START 0
#define DNAS_PROFILE_FROM_END 1
int dnas_pair_profiles(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                       const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                       int device_id, size_t arena_bytes, int32_t anchor, int64_t n_positions, double *out_profile,
                       int64_t *out_coverage, double *out_pair_profiles, double *out_pair_ll, uint8_t *out_status,
                       dnas_counts_stats *out_stats);
int dnas_pair_profiles_host(const dnas_mutator_params *params, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                            const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                            int exact_lse, int32_t anchor, int64_t n_positions, double *out_profile, int64_t *out_coverage,
                            double *out_pair_profiles, double *out_pair_ll, uint8_t *out_status);

/*
 * The EM of dnas_baum_welch (Laplace prior, mlParams with pLen back to uniform, at most 100 iterations, stop when ll + log
 * prior gains less than 1e-3 of itself) over dnas_pair_counts: the error model fitted from unaligned (original, read) pairs,
 * every alignment inside the band summed at every iteration.  Sequences, table and scratch go to the GPU once per fit.
 *   max_iterations         0: 100
 *   out_trace_params, out_trace_ll   may be NULL; else room for max_iterations (100 for 0) entries: the parameters of every
 *                          E-step that was run and its ll + log prior.  *out_n_trace (may be NULL): entries written
 * dnas_baum_welch_pairs_host runs the same loop (csrc/host/baumwelch.hpp) over dnas_pair_counts_host.
 */
int dnas_baum_welch_pairs(const dnas_mutator_params *init, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                          const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                          int device_id, size_t arena_bytes, int32_t max_iterations, dnas_mutator_params *out,
                          int32_t *out_iterations, dnas_mutator_params *out_trace_params, double *out_trace_ll,
                          int32_t *out_n_trace);
int dnas_baum_welch_pairs_host(const dnas_mutator_params *init, int32_t band, int64_t n_pairs, const int8_t *in_seqs,
                               const int64_t *in_off, const int8_t *out_seqs, const int64_t *out_off, const uint8_t *out_rev,
                               int exact_lse, int32_t max_iterations, dnas_mutator_params *out, int32_t *out_iterations,
                               dnas_mutator_params *out_trace_params, double *out_trace_ll, int32_t *out_n_trace);

/* ---- assigning the reads of a pool to their originals ------------------------------------ */

/*
 * dnas_align_pairs wants to be told which read belongs to which original; a sequencing run returns a shuffled pool, in either
 * orientation, from a library of K synthesised strands.  Read assignment finds, per read, the original and the orientation
 * under which the score S(I,O) of the model above is largest.  The reference has no counterpart.
 *
 * Inputs: the originals a_0 .. a_{K-1} and the reads b_0 .. b_{N-1}, concatenated as for dnas_align_pairs; a band with the
 * meaning it has there (DNAS_ALIGN_FULL included); a strand mode DNAS_STRAND_FORWARD | _REVERSE | _BOTH; optionally the
 * candidates of every read as a CSR list: read r's are cand_idx[cand_off[r] .. cand_off[r+1]), indices into the originals in
 * the order they are to be tried, duplicates allowed; cand_off = NULL: every original, in index order.
 *
 * The items of read r are its candidates in listed order; under DNAS_STRAND_BOTH each candidate is taken forward first, then
 * against the read's reverse complement (dnas_reverse_complement); under _REVERSE against the reverse complement only.  An
 * item's score is S(I,O) of dnas_align_pairs_host for (original, oriented read, band), bit for bit; -inf where there is no path.
 *   out_original[N]  the original of the best item: the first one, in item order, whose score is strictly greater than
 *                    every earlier item's and than -inf (the first-strictly-greater rule of every "best of" here); -1 if none
 *   out_strand[N]    1 if the best item is against the reverse complement, else 0 (0 where out_original is -1)
 *   out_score[N]     the best item's score (-inf where out_original is -1)
 *   out_second[N]    the largest score among the items whose original index differs from out_original (a duplicate of the
 *                    winner at another index counts, its other strand does not); -inf if there is none.  out_score -
 *                    out_second is the log-odds margin a caller thresholds on
 *   out_status[N]    DNAS_ASSIGN_OK, DNAS_ASSIGN_NO_PATH (there are items and all are -inf) or DNAS_ASSIGN_NO_CANDIDATES
 *   out_item_scores  may be NULL; else receives every item's score, reads in order, items in item order (the caller sizes it:
 *                    strands x candidates doubles per read) -- a testing and analysis aid
 * Host pointers.  Checks as for dnas_align_pairs (n_len > 13: DNAS_E_UNSUPPORTED; a base code outside 0..3: DNAS_E_BAD_BASE;
 * offsets), a cand_idx outside [0, K): DNAS_E_INVALID.  N = 0 and K = 0 are valid calls.
 *
 * dnas_assign_reads_host is the statement: one thread, dnas_align_pairs_host's recurrence per item and the fold above, no GPU.
 * The GPU entries are bit-identical to it whatever the device count, the grid and the chunking.  They keep no choice words and
 * trace nothing back: a score-only kernel walks the items, which it derives from its work index (no N x K list exists on the
 * host or in HBM), into one chunk of item scores of bounded size, and a second kernel folds the chunk into per-read state, chunk
 * after chunk in stream order.  The handle keeps the originals on the device between runs.  device_id = -1: the reads are
 * dealt over the GPUs of the node by their items x (read length + 1), costliest first in snake order, every device holding
 * every original, one host thread per device (DNAS_FAKE_DEVICES as for dnas_fb_create); results come back in the caller's
 * order.  Testing aids: DNAS_ASSIGN_CHUNK=n caps the chunk at n items, DNAS_ALIGN_BLOCKS=n the score kernel's grid.
 */
#define DNAS_ASSIGN_OK 0
#define DNAS_ASSIGN_NO_PATH 1
#define DNAS_ASSIGN_NO_CANDIDATES 2
typedef struct dnas_assign_stats {
  double score_ms, fold_ms;   /* summed kernel durations (HIP events); with several devices the slowest device's */
  int64_t items;              /* (read, candidate, strand) triples scored */
  int64_t cells;              /* cells inside the band, all items */
  int64_t chunks;             /* score-kernel launches (summed over the devices) */
} dnas_assign_stats;
typedef struct dnas_assigner dnas_assigner;
int dnas_assigner_create(const dnas_mutator_params *params, int32_t band, int64_t n_originals, const int8_t *orig_seqs,
                         const int64_t *orig_off, int device_id, dnas_assigner **out);
int dnas_assigner_run(dnas_assigner *h, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off, int strand_mode,
                      const int64_t *cand_off, const int64_t *cand_idx, int64_t *out_original, uint8_t *out_strand,
                      double *out_score, double *out_second, uint8_t *out_status, double *out_item_scores,
                      dnas_assign_stats *out_stats);
void dnas_assigner_destroy(dnas_assigner *h);
/* create, run, destroy */
int dnas_assign_reads(const dnas_mutator_params *params, int32_t band, int64_t n_originals, const int8_t *orig_seqs,
                      const int64_t *orig_off, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off, int strand_mode,
                      const int64_t *cand_off, const int64_t *cand_idx, int device_id, int64_t *out_original, uint8_t *out_strand,
                      double *out_score, double *out_second, uint8_t *out_status, double *out_item_scores,
                      dnas_assign_stats *out_stats);
int dnas_assign_reads_host(const dnas_mutator_params *params, int32_t band, int64_t n_originals, const int8_t *orig_seqs,
                           const int64_t *orig_off, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                           int strand_mode, const int64_t *cand_off, const int64_t *cand_idx, int64_t *out_original,
                           uint8_t *out_strand, double *out_score, double *out_second, uint8_t *out_status,
                           double *out_item_scores);

/* ---- one message per cluster of reads: consensus by rescoring ------------------------------ */

/*
 * A sequencing run returns several reads of every synthesised strand.  Given the reads of one strand (a cluster) and a few
 * candidate strands for it, the consensus is the candidate under which the reads are jointly most probable: the one with the
 * largest sum, over every read of the cluster, of the score S(I,O) of dnas_align_pairs.  The reference has no counterpart.
 *
 * Inputs: the error model and a band with the meaning they have for dnas_align_pairs (DNAS_ALIGN_FULL included); n_cand
 * candidate strands and n_reads reads, concatenated as there (cand_off[n_cand + 1], read_off[n_reads + 1]), both grouped by
 * cluster: cluster c owns the candidates cluster_cand_off[c] .. cluster_cand_off[c+1] - 1 and the reads cluster_read_off[c] ..
 * cluster_read_off[c+1] - 1 (both arrays have n_clusters + 1 entries, start at 0 and end at n_cand / n_reads); read_strand[n_reads],
 * or NULL for all zeros: 1 = the read is scored as its reverse complement (dnas_reverse_complement), 0 = as given.
 *
 * The items of a cluster are its (candidate j, read i) pairs, candidate-major: all reads of its first candidate in read order,
 * then those of its second.  An item's score is S(I,O) of dnas_align_pairs_host for (candidate, oriented read, band), bit for
 * bit; -inf where there is no path.  total[j] is the fp64 sum of candidate j's item scores, formed left to right in read order
 * starting from 0.0: one -inf item makes it -inf, a cluster without reads leaves it 0.0.
 *   out_status[n_clusters]  DNAS_CONSENSUS_NO_CANDIDATES (the cluster has no candidate), else DNAS_CONSENSUS_NO_READS (it has no
 *                           read), else DNAS_CONSENSUS_NO_PATH (every total is -inf), else DNAS_CONSENSUS_OK
 *   out_winner[n_clusters]  with DNAS_CONSENSUS_OK the first candidate of the cluster, in candidate order, whose total is strictly
 *                           greater than every earlier one's and than -inf (the first-strictly-greater rule of every "best of"
 *                           here), as an index into the call's candidates (0 .. n_cand - 1); -1 with every other status
 *   out_total[n_clusters]   the winner's total (-inf where out_winner is -1)
 *   out_second[n_clusters]  the largest total among the cluster's other candidates -- a copy of the winner's strand at another
 *                           index counts, the margin out_total - out_second is 0 then --; -inf if there is none
 *   out_totals              may be NULL; else double[n_cand], every candidate's total
 *   out_stats               may be NULL.  dnas_consensus_score fills score_ms .. chunks and candidates = n_cand
 * Host pointers.  Checks as for dnas_assign_reads: offsets that do not ascend or do not start at 0 and a read_strand above 1
 * are DNAS_E_INVALID, a base code outside 0..3 DNAS_E_BAD_BASE, n_len > 13 DNAS_E_UNSUPPORTED.  Zero clusters, candidates or
 * reads are valid calls.
 *
 * dnas_consensus_score_host is the statement: one thread, dnas_align_pairs_host's recurrence per item, the sums and the pick
 * above, no GPU.  dnas_consensus_score is bit-identical to it whatever the device count, the grid and the chunking.  Its score
 * kernel shares the cell update of dnas_align_pairs and dnas_assign_reads; a wave derives (cluster, candidate, read, strand) from
 * its work index by bisecting the per-cluster item offsets, so no expanded item list exists on the host or in HBM.  Scores go to
 * one chunk of at most 2^22 doubles -- the only device memory beyond the inputs and the per-candidate and per-cluster outputs --
 * which a second kernel adds, one thread per candidate in item order, to per-candidate totals; chunks follow each other in
 * stream order, so a candidate whose reads span chunks is summed in the order of the statement.  A last pass picks every
 * cluster's winner.  device_id = -1: the clusters are dealt over the GPUs of the node by candidates x sum over the reads of
 * (length + 1), costliest first in snake order, one host thread per device (DNAS_FAKE_DEVICES as for dnas_fb_create); results
 * come back in the caller's order and indices.  Testing aids: DNAS_CONSENSUS_CHUNK=n caps the chunk at n items,
 * DNAS_ALIGN_BLOCKS=n the score kernel's grid.
 */
#define DNAS_CONSENSUS_OK 0
#define DNAS_CONSENSUS_NO_PATH 1
#define DNAS_CONSENSUS_NO_CANDIDATES 2
#define DNAS_CONSENSUS_NO_READS 3
typedef struct dnas_consensus_stats {
  double score_ms, fold_ms;   /* summed kernel durations (HIP events); with several devices the slowest device's */
  int64_t items;              /* (candidate, read) pairs scored */
  int64_t cells;              /* cells inside the band, all items */
  int64_t chunks;             /* score-kernel launches (summed over the devices) */
  int64_t candidates;         /* candidate strands of the call (dnas_viterbi_clusters: the distinct strands it made) */
  int64_t encode_failures;    /* dnas_viterbi_clusters: decoded messages the encoder refused */
  double decode_wall_ms, candidates_wall_ms, rescore_wall_ms;   /* dnas_viterbi_clusters: host wall time of its three steps */
  double polish_wall_ms;      /* dnas_viterbi_clusters_ex: host wall time of the consensus reads and their decode (0 without) */
} dnas_consensus_stats;
int dnas_consensus_score(const dnas_mutator_params *params, int32_t band, int64_t n_clusters, int64_t n_cand,
                         const int8_t *cand_seqs, const int64_t *cand_off, const int64_t *cluster_cand_off, int64_t n_reads,
                         const int8_t *read_seqs, const int64_t *read_off, const uint8_t *read_strand,
                         const int64_t *cluster_read_off, int device_id, int64_t *out_winner, double *out_total,
                         double *out_second, uint8_t *out_status, double *out_totals, dnas_consensus_stats *out_stats);
int dnas_consensus_score_host(const dnas_mutator_params *params, int32_t band, int64_t n_clusters, int64_t n_cand,
                              const int8_t *cand_seqs, const int64_t *cand_off, const int64_t *cluster_cand_off, int64_t n_reads,
                              const int8_t *read_seqs, const int64_t *read_off, const uint8_t *read_strand,
                              const int64_t *cluster_read_off, int64_t *out_winner, double *out_total, double *out_second,
                              uint8_t *out_status, double *out_totals);
/*
 * The same with the item score named.  score_mode = DNAS_SCORE_VITERBI: exactly the two calls above.  DNAS_SCORE_FORWARD: an
 * item's score is the forward score of dnas_pair_likelihoods_host (table mode) for (candidate, oriented read, band), bit for
 * bit, so a total is the log-likelihood of the cluster's reads given the candidate; totals, the first-strictly-greater pick,
 * out_second and the statuses are defined as above.  The kernel is the score kernel built with the sum-product cell.
 *   out_posterior   may be NULL; else double[n_cand].  For a cluster with DNAS_CONSENSUS_OK candidate j gets
 *                   exp(total_j - Z), Z = m + log(sum_j exp(total_j - m)), m the cluster's largest total, the sum in candidate
 *                   order in fp64 (a -inf total gives 0): P(candidate | reads) under a prior that is uniform over the cluster's
 *                   LISTED candidates -- a strand listed twice counts twice and shares its mass equally.  0 for every candidate
 *                   of a cluster with any other status.  It is computed on the host from the per-candidate totals by both
 *                   entries, which therefore agree bit for bit.  With DNAS_SCORE_VITERBI a non-NULL out_posterior is
 *                   DNAS_E_INVALID: a Viterbi total is not a likelihood.  Any other score_mode is DNAS_E_INVALID.
 */
int dnas_consensus_score_ex(const dnas_mutator_params *params, int32_t band, int64_t n_clusters, int64_t n_cand,
                            const int8_t *cand_seqs, const int64_t *cand_off, const int64_t *cluster_cand_off, int64_t n_reads,
                            const int8_t *read_seqs, const int64_t *read_off, const uint8_t *read_strand,
                            const int64_t *cluster_read_off, int device_id, int score_mode, int64_t *out_winner,
                            double *out_total, double *out_second, uint8_t *out_status, double *out_totals,
                            double *out_posterior, dnas_consensus_stats *out_stats);
int dnas_consensus_score_host_ex(const dnas_mutator_params *params, int32_t band, int64_t n_clusters, int64_t n_cand,
                                 const int8_t *cand_seqs, const int64_t *cand_off, const int64_t *cluster_cand_off,
                                 int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off, const uint8_t *read_strand,
                                 const int64_t *cluster_read_off, int score_mode, int64_t *out_winner, double *out_total,
                                 double *out_second, uint8_t *out_status, double *out_totals, double *out_posterior);

/*
 * The decoder on top of it: clusters of reads in, one message per cluster out.  The candidates of a cluster are the messages
 * its own reads decode to; the right message must be among them, so at least one read of the cluster has to decode to it
 * (dnas_viterbi_clusters_ex below adds the message of a consensus read, which lifts that limit where the reads are noisy).
 *   1. dnas_viterbi_batch_strands over all reads in strand_mode: read_offsets, bases and the per-read outputs out_sym ..
 *      out_strand are that call's, with its conventions, and are returned as it fills them.
 *   2. Per cluster, the reads with DNAS_READ_OK and a non-empty message are walked in order and each message is encoded with
 *      dnas_encode_symbols; a message the encoder refuses is dropped and counted in encode_failures.  The distinct STRANDS, in
 *      order of first appearance, are the cluster's candidates (two messages that encode to one strand are one candidate);
 *      a candidate's proposer is the first read that produced its strand, its votes the number of reads whose messages encode
 *      to it.
 *   3. dnas_consensus_score on the model's device, with band and params (those the model was flattened with are the natural
 *      choice), every read of the cluster scored in the orientation step 1 decoded it in (out_strand).
 * Cluster c owns the reads cluster_read_off[c] .. cluster_read_off[c+1] - 1.  Per cluster:
 *   out_read[n_clusters]          the winner's proposer, an index into the call's reads; the cluster's message is that read's
 *                                 decoded symbols, out_sym[out_offsets[r] .. + out_len[r]), unchanged from step 1; -1: no winner
 *   out_total, out_second         as dnas_consensus_score
 *   out_n_candidates, out_votes   int32: the cluster's candidates, and the winner's votes (0 where out_read is -1)
 *   out_cluster_status            DNAS_CONSENSUS_*
 *   out_stats                     may be NULL; the decode's dnas_batch_stats and dnas_strand_stats stay readable through the model
 * dnas_model_device: the GPU a model lives on.
 */
int dnas_viterbi_clusters(dnas_model *model, const dnas_machine *machine, const dnas_mutator_params *params, int32_t band,
                          int64_t n_reads, const uint64_t *read_offsets, const uint8_t *bases, const int64_t *cluster_read_off,
                          int64_t n_clusters, int strand_mode, char *out_sym, const uint64_t *out_offsets, uint32_t *out_len,
                          double *out_loglike, uint8_t *out_status, uint8_t *out_strand, int64_t *out_read, double *out_total,
                          double *out_second, int32_t *out_n_candidates, int32_t *out_votes, uint8_t *out_cluster_status,
                          dnas_consensus_stats *out_stats);
int dnas_model_device(const dnas_model *model);

/* ---- consensus reads: a cluster column-voted under the pair HMM ---------------------------- */

/*
 * dnas_viterbi_clusters can only return a message one of the cluster's reads decodes to on its own.  A consensus read is a
 * sequence none of the reads may equal: every read of the cluster is aligned to a template and the alignments' columns vote on
 * every template position and every gap between two of them.  The reference has no counterpart.
 *
 * A cluster has a template t[0..I) and R reads, grouped as for dnas_consensus_score (template c is tmpl_seqs[tmpl_off[c] ..
 * tmpl_off[c+1]), the cluster owns the reads cluster_read_off[c] .. cluster_read_off[c+1] - 1, read_strand as there: 1 = the read
 * votes as its reverse complement).  One ROUND:
 *   1. Every oriented read is aligned to the template, the template as the original, exactly as dnas_align_pairs_host aligns
 *      (original, read, band).  A read whose status is not DNAS_ALIGN_OK does not vote; V is the number of voters.
 *   2. The op bytes of every voter are walked with ip = op = 0 (ip counts template bases, op read bases).  A match column adds 1
 *      to M[ip][out[op]].  A deletion column adds 1 to D[ip].  A maximal run of consecutive duplication columns -- whether they
 *      belong to one duplication or to several does not matter -- stands at gap g = ip; with b_0 .. b_{L-1} its read bases it
 *      adds, for each k < min(L, DNAS_POLISH_MAX_INSERT), 1 to N[g][k] and 1 to B[g][k][b_k]: longer runs are truncated.  All
 *      counters are integers.
 *   3. The new template is emitted for g = 0 .. I.  First the insertion at gap g: for k = 0, 1, ... while 2 * N[g][k] > V, the
 *      base with the largest B[g][k][.], on a tie the smallest code.  Then, if g < I and not 2 * D[g] > V, position g's base:
 *      t[g] if M[g][t[g]] equals the largest entry of M[g][.], otherwise the smallest code that reaches it.
 * Rounds repeat with the new template until
 *   - a round returns the template it was given: out_converged = 1; out_rounds counts the rounds that changed the template;
 *   - rounds_max rounds have run: out_converged = 0 (rounds_max = 0 returns the templates: no round runs, out_voters is 0);
 *   - V = 0: the template stays, DNAS_POLISH_NO_VOTERS, out_converged = 0;
 *   - the cluster has no reads: the template stays, DNAS_POLISH_NO_READS, out_converged = 0, no round runs.
 * Otherwise the status is DNAS_POLISH_OK.  out_voters and out_status are those of the last round that ran.
 *   out_seqs, out_off[n_clusters + 1]  the consensus reads, concatenated; *out_seqs is allocated by the library (dnas_free)
 *   out_rounds, out_voters             int32[n_clusters]
 *   out_converged, out_status          uint8[n_clusters]
 *   out_stats                          may be NULL
 * Host pointers.  Checks as for dnas_consensus_score (offsets that do not ascend: DNAS_E_INVALID, a base code outside 0..3:
 * DNAS_E_BAD_BASE, n_len > 13: DNAS_E_UNSUPPORTED); rounds_max < 0: DNAS_E_INVALID.  Zero clusters is a valid call.
 *
 * The votes are integers, so the result does not depend on the order the reads are met in: dnas_cluster_consensus_host (one
 * thread, dnas_align_pairs_host's aligner per pair, the walk and the emit above) is the statement, and dnas_cluster_consensus
 * equals it whatever the grid, the batching and the device count.  Per round the GPU fills the (template, read) pairs of the
 * clusters still changing with the recording fill of dnas_align_pairs -- a pair takes its template from its cluster, no
 * template is copied per read --, then a traceback that votes instead of writing op bytes adds into the cluster's table of 25
 * counters per template position with integer atomics, and the cluster's new template is emitted next to the old one.  A
 * template of up to 650 bases has its table in LDS (one work-group per cluster votes and emits, the table never exists in HBM),
 * a longer one in HBM.  No op byte leaves the chip; per round the host reads back the new lengths, the changed flags, the
 * voters and the new templates.  The choice words of a round live in an arena as for dnas_align_pairs (arena_bytes = 0: a
 * fraction of the free HBM) and the round runs in as many batches of whole clusters as the arena needs; a cluster whose
 * records alone exceed the arena is DNAS_E_INVALID.  device_id = -1: the clusters are dealt over the GPUs of the node by
 * (template length + 1) x the sum of their reads' lengths, costliest first in snake order, one host thread per device
 * (DNAS_FAKE_DEVICES as for dnas_fb_create); results come back in the caller's order.  Testing aids: DNAS_POLISH_LDS_POSITIONS=n
 * caps the LDS route at templates of n bases, DNAS_ALIGN_BLOCKS=n the fill's grid.
 */
#define DNAS_POLISH_MAX_INSERT 4
#define DNAS_POLISH_OK 0
#define DNAS_POLISH_NO_VOTERS 1
#define DNAS_POLISH_NO_READS 2
typedef struct dnas_polish_stats {
  double fill_ms, vote_ms;    /* summed kernel durations (HIP events); with several devices the slowest device's */
  int64_t rounds;             /* rounds launched (with several devices the largest number any device launched) */
  int64_t pairs;              /* (template, read) pairs filled, all rounds */
  int64_t cells;              /* cells inside the band, all pairs */
  int64_t batches;            /* fill launches (summed over the devices) */
  int64_t lds_clusters, hbm_clusters;   /* (cluster, round) pairs whose table was in LDS / in HBM */
} dnas_polish_stats;
int dnas_cluster_consensus(const dnas_mutator_params *params, int32_t band, int64_t n_clusters, const int8_t *tmpl_seqs,
                           const int64_t *tmpl_off, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                           const uint8_t *read_strand, const int64_t *cluster_read_off, int32_t rounds_max, int device_id,
                           size_t arena_bytes, int8_t **out_seqs, int64_t *out_off, int32_t *out_rounds, uint8_t *out_converged,
                           int32_t *out_voters, uint8_t *out_status, dnas_polish_stats *out_stats);
int dnas_cluster_consensus_host(const dnas_mutator_params *params, int32_t band, int64_t n_clusters, const int8_t *tmpl_seqs,
                                const int64_t *tmpl_off, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                                const uint8_t *read_strand, const int64_t *cluster_read_off, int32_t rounds_max,
                                int8_t **out_seqs, int64_t *out_off, int32_t *out_rounds, uint8_t *out_converged,
                                int32_t *out_voters, uint8_t *out_status);

/*
 * dnas_viterbi_clusters with a consensus read per cluster as one more source of candidates.  polish_rounds = 0 is
 * dnas_viterbi_clusters itself (out_source is all 0, out_cons_off all 0, nothing else of the extra outputs is touched, all of
 * them may be NULL).  With polish_rounds > 0, after step 1:
 *   1b. dnas_cluster_consensus on the model's device with band, params and rounds_max = polish_rounds: a cluster's template is its
 *       first read in the orientation step 1 decoded it in, its reads vote in theirs (out_strand).  The consensus reads are decoded
 *       with one dnas_viterbi_batch (they are oriented already).
 *   2'. The candidates of step 2; then the consensus read's message, if it decoded (DNAS_READ_OK, not empty), is encoded, and
 *       its strand, if it is not among the cluster's candidates yet, becomes the cluster's last candidate.  It has no proposer
 *       and no votes (votes count reads); a message the encoder refuses counts in encode_failures.
 *   3.  as before.  Where the extra candidate wins, out_read is -1, out_votes 0, out_source 1 and the cluster's message is the
 *       consensus read's decode.
 *   out_source[n_clusters]            0: the message is read out_read's (or there is none), 1: the consensus read's
 *   out_cons_seqs, out_cons_off       the consensus reads as dnas_cluster_consensus returns them (library-allocated, dnas_free)
 *   out_cons_sym, cons_sym_offsets,   their decodes with dnas_viterbi_batch's conventions: the caller sizes the slot of cluster c,
 *   out_cons_len, out_cons_loglike,   cons_sym_offsets[c + 1] - cons_sym_offsets[c]; a consensus read is at most polish_rounds x 2
 *   out_cons_status                   x the cluster's longest read longer than the first read
 * The model's dnas_batch_stats are then those of the consensus reads' decode.  out_stats: polish_wall_ms is the wall time of 1b.
 */
int dnas_viterbi_clusters_ex(dnas_model *model, const dnas_machine *machine, const dnas_mutator_params *params, int32_t band,
                             int64_t n_reads, const uint64_t *read_offsets, const uint8_t *bases, const int64_t *cluster_read_off,
                             int64_t n_clusters, int strand_mode, int32_t polish_rounds, char *out_sym,
                             const uint64_t *out_offsets, uint32_t *out_len, double *out_loglike, uint8_t *out_status,
                             uint8_t *out_strand, int64_t *out_read, double *out_total, double *out_second,
                             int32_t *out_n_candidates, int32_t *out_votes, uint8_t *out_cluster_status, uint8_t *out_source,
                             int8_t **out_cons_seqs, int64_t *out_cons_off, char *out_cons_sym, const uint64_t *cons_sym_offsets,
                             uint32_t *out_cons_len, double *out_cons_loglike, uint8_t *out_cons_status,
                             dnas_consensus_stats *out_stats);

/*
 * The same with the scorer of step 3 named: score_mode as for dnas_consensus_score_ex.  out_confidence[n_clusters] (may be
 * NULL; DNAS_E_INVALID with DNAS_SCORE_VITERBI): the winner's posterior among the cluster's candidates, 0 where the cluster has
 * no winner -- what a caller with an outer code thresholds to mark a doubtful strand as an erasure.  With DNAS_SCORE_VITERBI
 * and a NULL out_confidence this is dnas_viterbi_clusters_ex.
 */
int dnas_viterbi_clusters_scored(dnas_model *model, const dnas_machine *machine, const dnas_mutator_params *params, int32_t band,
                                 int64_t n_reads, const uint64_t *read_offsets, const uint8_t *bases,
                                 const int64_t *cluster_read_off, int64_t n_clusters, int strand_mode, int32_t polish_rounds,
                                 char *out_sym, const uint64_t *out_offsets, uint32_t *out_len, double *out_loglike,
                                 uint8_t *out_status, uint8_t *out_strand, int64_t *out_read, double *out_total,
                                 double *out_second, int32_t *out_n_candidates, int32_t *out_votes, uint8_t *out_cluster_status,
                                 uint8_t *out_source, int8_t **out_cons_seqs, int64_t *out_cons_off, char *out_cons_sym,
                                 const uint64_t *cons_sym_offsets, uint32_t *out_cons_len, double *out_cons_loglike,
                                 uint8_t *out_cons_status, int score_mode, double *out_confidence,
                                 dnas_consensus_stats *out_stats);

/* ---- forming the clusters: which reads of a pool are copies of one strand ------------------ */

/*
 * dnas_viterbi_clusters wants to be told which reads belong together; a decoding run has a pool of reads of either strand, no
 * originals and no labels.  dnas_cluster_reads partitions the pool into the connected components of a graph whose vertices are
 * the reads and whose edges are the pairs a k-mer sketch lets through and the pair-HMM score confirms.  Components do not depend
 * on the order the edges are found in: one GPU, several GPUs and the host statement agree bit for bit.  The reference has no
 * counterpart.
 *
 * 1. Sketch, with k in 1 .. 31 and m in {16, 32, 64}.  The code of the k-mer at position p of a read is f = sum over q < k of
 *    base[p+q] << 2 (k-1-q), that of its reverse complement r = the same sum over 3 - base[p+k-1-q], and c = min(f, r).  With
 *    mix64 the splitmix64 finaliser (x ^= x >> 30, x *= 0xBF58476D1CE4E5B9, x ^= x >> 27, x *= 0x94D049BB133111EB, x ^= x >> 31,
 *    all mod 2^64), sig[t] = the minimum over the read's k-mers of mix64(c + (t+1) * 0x9E3779B97F4A7C15) >> 32, for t < m.  A
 *    read and its reverse complement have one signature.  A read shorter than k has sig[t] = 0xFFFFFFFF for every t.
 * 2. Filter.  With min_shared >= 1 the pair (i, j), i < j, is a candidate when at least min_shared positions t have
 *    sig_i[t] == sig_j[t] != 0xFFFFFFFF.  With min_shared = 0 the filter is off (the exact mode): every pair of two non-empty
 *    reads is a candidate.  An empty read is never part of a candidate.
 * 3. Edge.  A candidate has two items: item 0 is S(I,O) of dnas_align_pairs_host for (read i, read j, band), bit for bit, item 1
 *    the same against the reverse complement of read j.  best is item 0 unless item 1 is strictly greater, strand says which.
 *    (i, j) is an edge iff best >= min_score_per_nt * (double)len_j: one fp64 multiply, one compare.  S is a log-odds against
 *    "read j is uniform random bases" (every substitution score has log 1/4 subtracted), so a floor of 0.0 is where "a mutated
 *    copy of read i" and "unrelated" explain read j equally well.
 * 4. Components.  Union-find with parity over the edges in (i, j) order.  Per read:
 *      out_root[N]     the smallest read index of its component
 *      out_cluster[N]  the component's dense id, ids given in order of first appearance (so in order of the roots)
 *      out_strand[N]   its orientation relative to the root: the XOR of the edge strands along the path (0 for a root)
 *      out_status[N]   DNAS_CLUSTER_EMPTY (length 0), else DNAS_CLUSTER_NO_SKETCH (shorter than k while min_shared >= 1), else
 *                      DNAS_CLUSTER_OK; reads of the first two kinds are components of their own
 *    An edge inside a component whose strand contradicts the orientations already fixed is counted in strand_conflicts and
 *    ignored.
 * out_edge_ij (2 int64 per edge), out_edge_score (best), out_edge_strand and out_n_edges may each be NULL; the arrays are
 * allocated by the library, sorted by (i, j), and freed with dnas_free.  out_stats may be NULL; the host statement fills the
 * counts and leaves the times 0.  Host pointers.  Checks as for dnas_assign_reads; k, m or min_shared out of range:
 * DNAS_E_INVALID; 2^31 reads or more: DNAS_E_UNSUPPORTED.  N = 0 is a valid call.
 *
 * dnas_cluster_reads_host is the statement: one thread, every pair through the filter, dnas_align_pairs_host's recurrence per
 * item, no GPU.  dnas_cluster_reads is bit-identical to it whatever the device count, the grid and the chunking: a kernel makes
 * the signatures (a wave per read), a tiled all-pairs compare of signatures counts every row's candidates and, after a prefix
 * sum, files them in (i, j) order band after band, the score kernel of dnas_assign_reads walks a band's list (two items per
 * pair), and a last kernel picks and tests every pair.  A band holds at most 2^21 pairs and may end inside a row.  Device memory
 * beyond the reads is N x m words of signatures, one band's list, scores and edges: nothing is of size N^2, though the filter
 * does compare N (N-1) / 2 pairs of signatures.  The edges are sorted and united on the host by the statement's own function.
 * device_id = -1: every device holds all reads and makes all signatures; the rows of the count pass and then the bands are dealt
 * over the devices, one host thread each (DNAS_FAKE_DEVICES as for dnas_fb_create).  Testing aids: DNAS_CLUSTER_CHUNK=n caps a
 * band at n pairs, DNAS_ALIGN_BLOCKS=n the score kernel's grid, DNAS_CLUSTER_GATE_WORDS=n the gate's register route (below).
 *
 * dnas_cluster_sketch_host: the signatures alone, out_sig[N * m].  dnas_cluster_candidates_host: every candidate in (i, j)
 * order with both item scores (out_cand_ij: 2 int64, out_cand_scores: 2 doubles per candidate; library-allocated, dnas_free) --
 * testing and analysis aids.
 */
#define DNAS_CLUSTER_OK 0
#define DNAS_CLUSTER_NO_SKETCH 1
#define DNAS_CLUSTER_EMPTY 2
typedef struct dnas_cluster_stats {
  double sketch_ms, filter_ms, score_ms, fold_ms;   /* summed kernel durations (HIP events); with several devices the slowest's */
  int64_t pairs;              /* N (N-1) / 2: the pairs of signatures the filter compares */
  int64_t candidates;         /* pairs the filter lets through */
  int64_t items;              /* (candidate, strand) pairs scored: 2 per candidate */
  int64_t cells;              /* cells inside the band, all items */
  int64_t edges;              /* candidates that reach the floor */
  int64_t chunks;             /* bands, which is score-kernel launches (summed over the devices) */
  int64_t clusters;           /* components */
  int64_t strand_conflicts;   /* edges ignored because their strand contradicts their component */
} dnas_cluster_stats;
int dnas_cluster_reads(const dnas_mutator_params *params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                       double min_score_per_nt, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off, int device_id,
                       int64_t *out_root, int64_t *out_cluster, uint8_t *out_strand, uint8_t *out_status, int64_t **out_edge_ij,
                       double **out_edge_score, uint8_t **out_edge_strand, int64_t *out_n_edges, dnas_cluster_stats *out_stats);
int dnas_cluster_reads_host(const dnas_mutator_params *params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                            double min_score_per_nt, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                            int64_t *out_root, int64_t *out_cluster, uint8_t *out_strand, uint8_t *out_status,
                            int64_t **out_edge_ij, double **out_edge_score, uint8_t **out_edge_strand, int64_t *out_n_edges,
                            dnas_cluster_stats *out_stats);
int dnas_cluster_sketch_host(int32_t k, int32_t m, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                             uint32_t *out_sig);
int dnas_cluster_candidates_host(const dnas_mutator_params *params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                                 int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off, int64_t **out_cand_ij,
                                 double **out_cand_scores, int64_t *out_n_cand);

/*
 * The edit-distance gate: a second, exact and cheap test between the sketch and the pair-HMM score.  A false candidate -- two
 * strands of one code that share a few k-mers -- is about 40 % apart, two noisy copies of one strand 10 - 25 %.
 *
 *   d(a, b)      the Levenshtein distance over base codes 0..3 (substitution, insertion, deletion, cost 1 each); d("", b) = len(b)
 *   e[0], e[1]   of a candidate (i, j): d(read i, read j) and d(read i, reverse complement of read j)
 *   limit(i, j)  (max_edit_permille * max(len_i, len_j)) / 1000 in int64, rounded down
 *   the gate     candidate (i, j) passes iff min(e[0], e[1]) <= limit(i, j)
 * A candidate that passes has both items scored exactly as without the gate: its best score, strand and floor test are those of
 * dnas_cluster_reads.  A candidate that fails is not scored and is no edge.  So the edges of a gated call are the ungated call's
 * edges, bit for bit, minus those whose candidate fails, and the components follow from the edges as before.
 * max_edit_permille = -1: no gate (dnas_cluster_reads[_host] are dnas_cluster_reads_gated[_host] with -1).  The range is
 * -1 .. 1000, anything else DNAS_E_INVALID; at 1000 every candidate passes.  All of it is integer arithmetic: the result does not
 * depend on the grid, the batching, the order of the survivors or the device count.
 *
 * With the gate on dnas_cluster_stats keeps its layout and meanings: candidates is what the sketch lets through, items = 2 *
 * passed, cells counts the passed pairs only, chunks the score launches (a band without a survivor launches none).  out_gate may
 * be NULL; the host statement fills the counts and leaves gate_ms 0.  Without the gate *out_gate is all 0.
 *
 * dnas_edit_distances: the gate's kernels as a primitive.  Pair q is (pair_ij[2q], pair_ij[2q+1]), two indices into the reads
 * (i = j is allowed, as is any order); out_dist[2q] = e[0], out_dist[2q+1] = e[1], exact, with no cutoff.  Checks as for
 * dnas_cluster_reads, and an index outside 0 .. n_reads - 1 is DNAS_E_INVALID; n_pairs = 0 is a valid call.  device_id = -1 deals
 * the pairs over the devices.  dnas_edit_distances_host is the statement: the two-row dynamic program, one thread.
 *
 * The kernels: one thread per pair runs Myers' bit-vector recurrence in its block form (Hyyro) for both orientations at once,
 * the shorter read as the pattern (words of 64 rows in registers, its match masks in LDS), the longer as the text, read from its
 * end with 3 - b for the second orientation.  A pattern of more than 512 rows takes the long route (masks and vectors in device
 * memory), which works for any length.  Testing aid: DNAS_CLUSTER_GATE_WORDS=n caps the register route at n words (0 .. 8); 0
 * sends every pair to the long route.
 */
typedef struct dnas_cluster_gate_stats {
  double gate_ms;             /* the gate's kernels, compaction included (HIP events); with several devices the slowest's */
  int64_t tested;             /* candidates put through the gate */
  int64_t passed;             /* ... that passed */
  int64_t long_pairs;         /* ... whose shorter read has more than 512 bases (the long route, unless the testing aid moves it) */
  int64_t word_steps;         /* sum over the tested candidates of 2 x 64-row words of the shorter read x bases of the longer */
} dnas_cluster_gate_stats;
int dnas_cluster_reads_gated(const dnas_mutator_params *params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                             double min_score_per_nt, int32_t max_edit_permille, int64_t n_reads, const int8_t *read_seqs,
                             const int64_t *read_off, int device_id, int64_t *out_root, int64_t *out_cluster, uint8_t *out_strand,
                             uint8_t *out_status, int64_t **out_edge_ij, double **out_edge_score, uint8_t **out_edge_strand,
                             int64_t *out_n_edges, dnas_cluster_stats *out_stats, dnas_cluster_gate_stats *out_gate);
int dnas_cluster_reads_gated_host(const dnas_mutator_params *params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                                  double min_score_per_nt, int32_t max_edit_permille, int64_t n_reads, const int8_t *read_seqs,
                                  const int64_t *read_off, int64_t *out_root, int64_t *out_cluster, uint8_t *out_strand,
                                  uint8_t *out_status, int64_t **out_edge_ij, double **out_edge_score, uint8_t **out_edge_strand,
                                  int64_t *out_n_edges, dnas_cluster_stats *out_stats, dnas_cluster_gate_stats *out_gate);
int dnas_edit_distances(int64_t n_pairs, const int64_t *pair_ij, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                        int device_id, int32_t *out_dist);
int dnas_edit_distances_host(int64_t n_pairs, const int64_t *pair_ij, int64_t n_reads, const int8_t *read_seqs,
                             const int64_t *read_off, int32_t *out_dist);

/*
 * A pool that grows: the persistent clusterer.  A sequencing run delivers its reads file by file; dnas_clusterer holds the pool
 * on one device between the deliveries, so that an add pays for the pairs it brings and for nothing that was settled before.
 *
 *   create   the parameters of dnas_cluster_reads_gated, checked as there and before any device is touched: a bad band, k, m,
 *            min_shared (negative, or more than m) or max_edit_permille is DNAS_E_INVALID on a machine without a GPU, as is a NULL
 *            out.  device_id = -1 is DNAS_E_UNSUPPORTED: a handle lives on one device.
 *   add      reads are numbered in order of arrival: an add that finds N0 reads in the handle gives its reads the indices
 *            N0 .. N1 - 1 and examines exactly the pairs (i, j), i < j, N0 <= j < N1 -- every pair whose larger index is new.  A
 *            pair is treated as dnas_cluster_reads_gated treats it: the candidate test on the two signatures, the gate when
 *            max_edit_permille >= 0, items 0 and 1 with read j as the mutated copy of read i, the pick against
 *            min_score_per_nt * len_j.  read_off starts at 0 for every add.  Offsets and base codes are checked as there
 *            (DNAS_E_INVALID, DNAS_E_BAD_BASE, a read that is too long or a total of 2^31 reads or more DNAS_E_UNSUPPORTED), all
 *            of it before any state changes: an add that is refused leaves the handle exactly as it was.  n_reads = 0 is a valid
 *            add that does nothing.  out_stats and out_gate (each may be NULL) describe this add alone: pairs = N_new * N0 +
 *            N_new (N_new - 1) / 2, clusters and strand_conflicts are left 0.
 *   reads    the reads held so far.
 *   result   the whole pool so far, with the outputs of dnas_cluster_reads_gated (out_root .. out_status sized by
 *            dnas_clusterer_reads): all edges sorted by (i, j), then the union of step 4 over them, by the statement's own
 *            function.  It may be called after any add, any number of times, and changes nothing in the handle.  On an empty
 *            handle it is the N = 0 answer of the one-shot call.
 *   destroy  frees the handle (NULL is allowed).
 *
 * The contract: after the adds B1 .. Bk every output of dnas_clusterer_result equals that of dnas_cluster_reads_gated_host on the
 * concatenation B1 || .. || Bk, bit for bit -- root, cluster, strand, status, the edge list with its score bits and strands, the
 * counts pairs, candidates, items, cells, edges, clusters, strand_conflicts and the gate's tested, passed, long_pairs and
 * word_steps -- whatever the batch boundaries, the grid and the band size: every test is a function of one pair of reads, and
 * the components do not depend on the order the edges are found in.  The result's stats are the sums over the adds (chunks: the
 * summed launches; the times: summed), clusters and strand_conflicts come from the union.
 *
 * The handle keeps on its device the reads, their offsets and signatures, one band's list, scores and edges, and the gate's
 * buffers; no old read is uploaded or sketched twice.  The first add allocates what it needs, a later one grows a buffer that is
 * too small to max(needed, 2 x its capacity) with a device-to-device copy.  The edges found so far live on the host.  The filter
 * of an add is column-owned: a work-group holds 64 new reads and lets the row tiles of every read in front of them pass by, cut
 * into row segments so that a small batch still fills the chip; counts per (column, segment) and a prefix sum on the host put
 * the add's candidates in (j, i) order with no sort and no atomic, band after band.  Behind the list the kernels are those of
 * dnas_cluster_reads_gated.  A device error in the middle of an add poisons the handle: every later add and result returns
 * DNAS_E_DEVICE, partial state is never served.  A handle is used by one thread at a time.  Testing aids: those of
 * dnas_cluster_reads, and DNAS_CLUSTERER_SEGMENTS=n forces the number of row segments.
 */
typedef struct dnas_clusterer dnas_clusterer;
int dnas_clusterer_create(const dnas_mutator_params *params, int32_t band, int32_t k, int32_t m, int32_t min_shared,
                          double min_score_per_nt, int32_t max_edit_permille, int device_id, dnas_clusterer **out);
int dnas_clusterer_add(dnas_clusterer *h, int64_t n_reads, const int8_t *read_seqs, const int64_t *read_off,
                       dnas_cluster_stats *out_stats, dnas_cluster_gate_stats *out_gate);
int64_t dnas_clusterer_reads(const dnas_clusterer *h);
int dnas_clusterer_result(dnas_clusterer *h, int64_t *out_root, int64_t *out_cluster, uint8_t *out_strand, uint8_t *out_status,
                          int64_t **out_edge_ij, double **out_edge_score, uint8_t **out_edge_strand, int64_t *out_n_edges,
                          dnas_cluster_stats *out_stats, dnas_cluster_gate_stats *out_gate);
void dnas_clusterer_destroy(dnas_clusterer *h);

/*
 * Demultiplexing and trimming: the front of the pipeline.  A synthesised molecule is forward primer . payload . reverse primer
 * with a few bases of adapter or junk around it, and the primer pair names the file it belongs to.  dnas_trim_reads finds, for
 * every read of a pool, the primer pair and strand that frame it best and where the payload begins and ends; every other call of
 * this library takes the payload.
 *
 * Base codes 0..3, rc the reverse complement.  Primer pair k is (F_k, R_k), both written as they appear on the forward strand:
 * the molecule is F_k . payload . R_k.  primer_seqs / primer_off hold 2 n_pairs sequences F_0, R_0, F_1, R_1, ...; each primer
 * has 1 .. 64 bases.
 *
 *   The search.  For a pattern p of m rows and a text t: D[0][c] = 0, D[r][0] = r, Levenshtein steps of cost 1; E[c] = D[m][c] for
 *   c = 0 .. w, where w = min(len t, m + max_offset), or len t when max_offset = -1.  search(p, t) = (e, c): e is the smallest E[c]
 *   and c the LARGEST column that attains it (a primer whose last base was substituted or deleted ties between two ends; the
 *   farther one leaves no primer base in the payload).
 *
 *   The candidates.  A read of n bases has one candidate per pair k and strand s (0: v = the read as given, 1: v = rc(read)):
 *   (eF, cF) = search(F_k, v), (eR, cR) = search(reverse(R_k), reverse(v)); its payload is v[cF : n - cR].  An anchor of m bases
 *   is within its limit iff e <= (max_edit_permille * m) / 1000, in int64, rounded down.
 *     anchors = DNAS_TRIM_BOTH:    the candidate is accepted iff both anchors are within their limits and
 *                                  cF + cR + min_payload <= n; its total is eF + eR.
 *     anchors = DNAS_TRIM_EITHER:  at least one anchor must be within its limit (truncated reads).  An anchor that is not is
 *                                  missing: it has c = 0, is reported as -1 edits and adds limit + 1 to the total.  The length test
 *                                  is the same.
 *
 *   The result per read.  The winner is the accepted candidate that is smallest by (total, k, s).
 *     out_pair    k of the winner, -1 without one
 *     out_strand  s of the winner (0 without one)
 *     out_begin, out_end   in the coordinates of the read as given: for s = 0 the payload is read[begin:end] with begin = cF,
 *                 end = n - cR; for s = 1 it is rc(read[begin:end]) with begin = cR, end = n - cF.  0, 0 without a winner.
 *     out_edits   [2 i], [2 i + 1] = eF, eR of the winner (-1: a missing anchor, or no winner)
 *     out_second  the smallest total among the accepted candidates of ANOTHER pair, -1 when there is none or no winner: what a
 *                 caller tests to ask for a margin
 *     out_status  DNAS_TRIM_OK; DNAS_TRIM_NO_ANCHOR: no candidate had its anchors within their limits; DNAS_TRIM_TOO_SHORT: some
 *                 candidate had, but none passed the length test
 *   A lexicographic minimum is associative and everything is integer arithmetic: the result does not depend on how pairs or reads
 *   are cut into work, on the grid or on the device count.
 *
 * Host pointers.  DNAS_E_INVALID: a primer of 0 or more than 64 bases, max_edit_permille outside 0 .. 1000, max_offset < -1,
 * anchors not 0 or 1, min_payload < 0, null pointers, offsets that do not ascend, a device_id that names no device (as for
 * dnas_edit_distances).  A base code outside 0..3: DNAS_E_BAD_BASE; 2^30 pairs, 2^31 reads or a read of 2^30 bases:
 * DNAS_E_UNSUPPORTED.  n_reads = 0 is a valid call, as is n_pairs = 0, where every read gets DNAS_TRIM_NO_ANCHOR.
 *
 * dnas_trim_reads_host is the statement and the CPU baseline: the two-row dynamic program of the search, one thread, no bit
 * vectors.  dnas_trim_reads is bit-identical to it.  The kernels (csrc/trim_kernels.hip): a thread per read, a wave of 64 reads
 * walks a chunk of the pairs with k wave-uniform.  The search is Myers' bit-vector recurrence with no +1 handed into the word
 * (gateBlock of cluster_gate.hpp with hin = 0), a primer one 64-bit word.  A pair has two mask sets, F and reverse(R), in a table
 * built once per call, of which every lane of the wave reads the same 72 bytes; each serves two of the four searches (F with base b on the read's front and
 * with 3 - b on its end read backwards, reverse(R) the mirror image), and all four advance in one loop over the columns.  The
 * read's two windows are packed 16 bases to a dword by a kernel of their own, [dword][read], so that the loads of a wave are
 * contiguous.  When the reads alone do not fill the chip the pairs are cut into chunks -- an item is (64 reads, pair chunk) -- and
 * a second kernel folds the chunks' states (the best candidate and the best total of another pair) in the (total, k, s) order.
 * device_id = -1 deals the reads over the devices by their window columns.  Testing aids: DNAS_TRIM_PAIR_CHUNK=n forces the
 * pairs of a chunk, DNAS_FAKE_DEVICES as elsewhere.
 */
#define DNAS_TRIM_BOTH 0
#define DNAS_TRIM_EITHER 1
#define DNAS_TRIM_OK 0
#define DNAS_TRIM_NO_ANCHOR 1
#define DNAS_TRIM_TOO_SHORT 2
typedef struct dnas_trim_stats {
  double kernel_ms;           /* pack, search and fold kernels (HIP events); with several devices the slowest's */
  int64_t items;              /* (64 reads, pair chunk) items */
  int64_t columns;            /* text columns walked: the sum over reads and pairs of 2 (w(F_k) + w(R_k)) */
  int64_t trimmed;            /* reads with DNAS_TRIM_OK */
  int64_t chunks;             /* pair chunks (the largest number on any device) */
  int64_t devices;
} dnas_trim_stats;
int dnas_trim_reads(int64_t n_pairs, const int8_t *primer_seqs, const int64_t *primer_off, int64_t n_reads, const int8_t *read_seqs,
                    const int64_t *read_off, int32_t max_offset, int32_t max_edit_permille, int32_t anchors, int32_t min_payload,
                    int device_id, int32_t *out_pair, uint8_t *out_strand, int32_t *out_begin, int32_t *out_end, int32_t *out_edits,
                    int32_t *out_second, uint8_t *out_status, dnas_trim_stats *out_stats);
int dnas_trim_reads_host(int64_t n_pairs, const int8_t *primer_seqs, const int64_t *primer_off, int64_t n_reads,
                         const int8_t *read_seqs, const int64_t *read_off, int32_t max_offset, int32_t max_edit_permille,
                         int32_t anchors, int32_t min_payload, int32_t *out_pair, uint8_t *out_strand, int32_t *out_begin,
                         int32_t *out_end, int32_t *out_edits, int32_t *out_second, uint8_t *out_status);

/* ---- simulating reads: the channel itself --------------------------------------------------- */

/*
 * Every call above takes reads; this one makes them.  dnas_simulate_reads samples reads of given strands from the mutator pair
 * HMM that the kernels score, and hands out the path with each read.  The result is fixed by the seed and nothing else.  The
 * reference has no counterpart (its simulator is the Perl of doc/errdecode.pl).
 *
 * Randomness.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85).  The key is the two
 * halves of seed (low, high); the counter is (c, position, read low, read high), read = first_index + the read's index in the
 * call, position the input position ip, or 0xFFFFFFFF for the per-read draws, c = 0, 1, ... the call within (read, position).
 * Call c yields the words w0..w3; draw 2c is ((w0 | w1 << 32) >> 11) * 2^-53, draw 2c + 1 is ((w2 | w3 << 32) >> 11) * 2^-53.  A
 * draw depends on (seed, read, position, j) only: not on the grid, the batches, the devices or how a caller splits its list.
 * dnas_simulate_draw_bits returns the 53 bits of a draw.
 *
 * Thresholds, sums formed once on the host, left to right in fp64; no transcendental function runs anywhere:
 *   tDel = pDelOpen, tDup = pDelOpen + pTanDup, cum[k] = pLen[0] + ... + pLen[k],
 *   substitution: pTransition, pTransition + pTransversion / 2, pTransition + pTransversion.
 *
 * Per position.  Input positions ip = 0 .. I are visited in order (I included: trailing duplications); a position is entered in
 * state S or D, position 0 in S; its draws are numbered j = 0, 1, ...
 *   Entered in D: at ip == I the deletion ends (draw 0 ignored); else draw 0 < pDelExtend makes a deletion column (op byte 1,
 *     n = 0), emits nothing more and leaves in D; any other draw 0 ends the deletion and the S loop runs.  A position entered
 *     in S never looks at draw 0.
 *   The S loop, from j = 1.  A duplication is possible when n = min(ip, P) > 0 and cum[n-1] > 0.  Take draw u:
 *     u < tDel and ip < I: a deletion column with n = 1; the position leaves in D.
 *     tDel <= u < tDup, a duplication possible, and fewer than 16 duplications so far at this position: the next draw v picks the
 *       first k < n with v * cum[n-1] < cum[k] (k = n - 1 if none); for t = k .. 0 a copy of in[ip-1-t] is emitted, each through
 *       a substitution draw of its own: k + 1 duplication columns, the first with n = k + 1; the loop goes on.
 *     anything else, ip < I: in[ip] is emitted through a substitution draw, a match column; the position leaves in S.
 *     anything else, ip == I: the read ends.
 *   A substitution draw of source base x emits x ^ 2 (its transition partner) below the first threshold, the smaller of the two
 *   other codes below the second, the larger below the third, else x.
 *
 * Ops and orientation.  The op bytes are those of dnas_align_pairs (kind | n << 2); dnas_alignment_expand and
 * dnas_stockholm_write take them as they are.  The per-read draw (0xFFFFFFFF, 0) below reverse_prob: the read is handed out
 * reverse-complemented and out_reversed is 1; the ops describe the read before that.  params->local is ignored: reads are whole.
 *
 * Where the sampler is not the pair HMM.  The pair HMM is not normalised at its edges (no duplication longer than ip; at ip == I
 * duplications only), so: a draw in the duplication interval that cannot be taken counts as a match; near the start the length
 * is drawn from pLen truncated to min(ip, P) entries; at ip == I everything but a duplication ends the read; a position makes
 * at most 16 duplications; a deletion that reaches I ends there without a draw (the model charges delEnd).
 *
 * Outputs, allocated by the library and released with dnas_free: *out_seqs / *out_off[n_reads + 1] the reads, *out_reversed
 * [n_reads], and with want_ops != 0 *out_ops / *out_ops_off[n_reads + 1] (else both NULL); out_status[n_reads] is the caller's:
 * DNAS_SIM_OK, or DNAS_SIM_TOO_LARGE for a read whose bases (and ops) alone exceed the arena -- it has length 0 and no ops, the
 * other reads are as without it.  out_stats may be NULL.
 * DNAS_E_INVALID: a probability (pLen included) or reverse_prob outside [0, 1], pDelOpen + pTanDup > 1, pTransition +
 * pTransversion > 1, a read_strand outside 0 .. n_strands - 1; a base code outside 0..3: DNAS_E_BAD_BASE; n_len > 32, a strand of
 * more than 2^20 bases or 2^31 reads: DNAS_E_UNSUPPORTED.  n_reads = 0 and empty strands are valid.
 *
 * dnas_simulate_reads_host is the statement: one thread, the positions in order, no GPU; never DNAS_SIM_TOO_LARGE.
 * dnas_simulate_reads is bit-identical to it (csrc/simulate_kernels.hip): a wave takes a read, its lanes the positions 64 chunk +
 * lane; every lane runs its position's S loop, two ballots (opens a deletion, draw 0 extends) and a carry bit from chunk to
 * chunk say which positions a deletion swallows, a wave-wide prefix sum places each lane's bases and ops.  Two passes over a
 * persistent grid: the first stores a read's totals, the host's exclusive scan of them gives offsets and batches, the second draws
 * the same numbers again and writes.  arena_bytes: the device buffer of a batch's bases and ops, 0 = half of the free HBM at most;
 * the call runs in as many batches as that needs.  device_id = -1 deals the reads over the devices by strand length
 * (DNAS_FAKE_DEVICES as elsewhere); the result does not depend on it.  DNAS_SIMULATE_BLOCKS=n (testing aid) caps the grid at n
 * work-groups of four waves; DNAS_SIMULATE_THREAD_PER_READ=1 runs the two passes with a thread per read instead, the layout the
 * shipped one is measured against (same result, never the default).
 */
#define DNAS_SIM_OK 0
#define DNAS_SIM_TOO_LARGE 1
typedef struct dnas_simulate_stats {
  double count_ms, write_ms;  /* the two passes' kernels (HIP events), summed over the batches; with several devices the slowest's */
  int64_t batches;            /* launches of the second pass (summed over the devices) */
  int64_t bases_in;           /* strand bases visited, all reads */
  int64_t bases_out, ops;     /* read bases and op bytes handed out */
  int64_t reads_too_large;
  int64_t devices;
} dnas_simulate_stats;
int dnas_simulate_reads(const dnas_mutator_params *params, int64_t n_strands, const int8_t *strand_seqs, const int64_t *strand_off,
                        int64_t n_reads, const int64_t *read_strand, uint64_t seed, uint64_t first_index, double reverse_prob,
                        int want_ops, int device_id, size_t arena_bytes, int8_t **out_seqs, int64_t **out_off, uint8_t **out_reversed,
                        uint8_t **out_ops, int64_t **out_ops_off, uint8_t *out_status, dnas_simulate_stats *out_stats);
int dnas_simulate_reads_host(const dnas_mutator_params *params, int64_t n_strands, const int8_t *strand_seqs,
                             const int64_t *strand_off, int64_t n_reads, const int64_t *read_strand, uint64_t seed,
                             uint64_t first_index, double reverse_prob, int want_ops, int8_t **out_seqs, int64_t **out_off,
                             uint8_t **out_reversed, uint8_t **out_ops, int64_t **out_ops_off, uint8_t *out_status);
uint64_t dnas_simulate_draw_bits(uint64_t seed, uint64_t read, uint32_t position, uint32_t j);

/* ---- the outer code: Reed-Solomon across the strands of a block ------------------------------ */

/*
 * Every call above ends with one message per strand; this one makes a file of them again.  A strand that was lost, or that
 * decoded to the wrong message, is repaired from the other strands of its block.  The reference has no counterpart.
 *
 * The code.  GF(2^8) modulo x^8 + x^4 + x^3 + x^2 + 1 (0x11d), alpha = 2.  RS(n, k): 2 <= n <= 255, 1 <= k < n, r = n - k <= 64
 * (a wave holds a syndrome per lane; anything else is DNAS_E_UNSUPPORTED).  A word c_0 .. c_{n-1} is read as c_0 x^(n-1) + ... +
 * c_{n-1}; it is a codeword iff it vanishes at alpha^0 .. alpha^(r-1).  Systematic: positions 0 .. k-1 are data, positions k ..
 * n-1 the remainder of data x^r modulo g(x) = prod (x - alpha^i).  (g for r = 7 has the exponents 0, 87, 229, 146, 149, 238, 102,
 * 21, as in the QR-code standard.)
 *
 * A block is n strands of L >= 1 bytes, strand-major uint8[n][L]: column j, byte j of every strand, is one codeword.  A call
 * holds B >= 0 blocks, uint8[B][n][L], and present uint8[B][n] (0: the strand is an erasure), so the L columns of a block share
 * one erasure set.  dnas_rs_encode takes the data strands uint8[B][k][L].
 *
 * The decoding rule, for one column with f erased positions.  If f <= r and a codeword exists that differs from the received
 * word in e present positions with 2 e + f <= r, that codeword is unique and is the output; out_status is DNAS_RS_OK (e = 0) or
 * DNAS_RS_CORRECTED (e > 0).  Otherwise -- always when f > r -- out_status is DNAS_RS_FAILED and the output is the received byte
 * at the present positions, 0 at the erased ones.  Bytes stored at erased positions are never read into the answer.
 *   out_blocks  [B][n][L]
 *   out_status  [B][L]
 *   out_errors  [B][L]  e, 0 for a failed column
 *   out_fixed   [B][n]  the DNAS_RS_CORRECTED columns of the block in which present strand p was changed: which strand was wrong
 * The rule defines the answer and field arithmetic is exact: the result does not depend on the algorithm, the grid, the
 * launches or the device count.
 *
 * dnas_rs_encode_host / dnas_rs_decode_host are the statement and the CPU baseline: one thread, long division, and per column
 * erasure locator -> Forney syndromes -> Berlekamp-Massey -> root search over the n positions -> Forney values, accepted only if
 * the root count equals the locator's degree, the corrected word's syndromes are zero and 2 e + f <= r (the re-check is what
 * makes DNAS_RS_FAILED follow the rule for shortened codes, whose locators can have roots outside the n positions).
 * dnas_rs_encode / dnas_rs_decode are byte-identical to them (csrc/rs_kernels.hip): a work-group takes a block and a tile of up
 * to 128 columns, loaded row by row into LDS; the erasure locator and the value denominators are computed once per work-group;
 * syndromes, the product with the locator and the erasure values are uniform loops in which four columns share a dword and a
 * multiplication by a constant is eight masked XORs of its doublings; only the columns whose Forney syndromes are not all zero go
 * through the solver, a thread each, after those loops.  Encoding runs the same kernel with the parity positions as the erasures.
 * device_id = -1 deals contiguous ranges of blocks over the devices (DNAS_FAKE_DEVICES as elsewhere); DNAS_RS_CHUNK=n (testing
 * aid) caps the blocks of a launch.  DNAS_E_INVALID: L < 1, B < 0, null pointers, a device_id that names no device.
 */
#define DNAS_RS_OK 0
#define DNAS_RS_CORRECTED 1
#define DNAS_RS_FAILED 2
typedef struct dnas_rs_stats {
  double kernel_ms;           /* the kernel (HIP events), summed over the launches; with several devices the slowest's */
  int64_t columns;            /* B L */
  int64_t columns_solved;     /* columns that went through the solver: their Forney syndromes were not all zero */
  int64_t launches;
  int64_t devices;
} dnas_rs_stats;
int dnas_rs_encode(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t *data, uint8_t *out_blocks, dnas_rs_stats *out_stats,
                   int device_id);
int dnas_rs_decode(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t *blocks, const uint8_t *present, uint8_t *out_blocks,
                   uint8_t *out_status, uint8_t *out_errors, int32_t *out_fixed, dnas_rs_stats *out_stats, int device_id);
int dnas_rs_encode_host(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t *data, uint8_t *out_blocks);
int dnas_rs_decode_host(int32_t n, int32_t k, int32_t L, int64_t B, const uint8_t *blocks, const uint8_t *present,
                        uint8_t *out_blocks, uint8_t *out_status, uint8_t *out_errors, int32_t *out_fixed);

/*
 * The strand frame and the file layer over the code.
 *   Record  4 + L bytes per strand: bytes 0..2 the strand number s = block n + position, big-endian; byte 3 a CRC-8 (polynomial
 *           0x07, initial value 0, not reflected) over bytes 0..2 and the L body bytes; then the body, the strand's row of its
 *           block.  dnas_outer_frame writes one, dnas_outer_crc8 is the CRC.
 *   Stream  the file's length as 8 bytes little-endian, the file, zeros up to B k L, B = ceil((8 + len) / (k L)) =
 *           dnas_outer_blocks; data strand (b, p < k) carries stream[(b k + p) L : +L].
 * dnas_outer_encode -> *out_n_blocks and the B n records one after the other (*out_records, released with dnas_free).
 * dnas_outer_decode takes any pool of records (record_bytes / record_off[n_records + 1]) and weights (NULL: all 1; finite, >= 0).
 *   A record is valid iff its length is 4 + L, its CRC matches and s < B n; otherwise it is dropped.  Per slot s identical
 *   records form a group, whose weight is the sum of its records' weights added in record order; the heaviest group wins; if the
 *   two heaviest groups tie, or the slot has no record, the slot is an erasure.  The blocks then go through dnas_rs_decode on
 *   device_id, or through dnas_rs_decode_host when host != 0.  A CRC-8 passes one corrupt record in 256 and a confident wrong
 *   consensus passes too: those are the errors the code corrects.
 *   out_present [B n], out_column_status [B L], out_fixed [B n]: the caller's.  *out_data / *out_len, *out_failed_ranges
 *   [2 *out_n_ranges] (begin, end pairs, ascending): the library's, released with dnas_free.
 *   *out_status  DNAS_OUTER_OK: the file.  DNAS_OUTER_DAMAGED: the file, but the named byte ranges of it lie in failed columns
 *   and hold what was received.  DNAS_OUTER_NO_LENGTH: a column that holds the length prefix failed; DNAS_OUTER_BAD_LENGTH: the
 *   length exceeds the stream -- in both cases *out_data is the raw stream of B k L bytes and the ranges are in its coordinates.
 * DNAS_E_UNSUPPORTED: B n beyond 2^24 (a strand number has three bytes), and whatever the code refuses.
 */
#define DNAS_OUTER_OK 0
#define DNAS_OUTER_DAMAGED 1
#define DNAS_OUTER_NO_LENGTH 2
#define DNAS_OUTER_BAD_LENGTH 3
typedef struct dnas_outer_stats {
  int64_t records, dropped;   /* records given; dropped as invalid */
  int64_t conflicts, ties;    /* slots with more than one group; of those, erased by a tie */
  int64_t erased;             /* slots without a winner */
  int64_t columns_ok, columns_corrected, columns_failed;
  int64_t strands_fixed;      /* strands with out_fixed != 0 */
  dnas_rs_stats rs;           /* of the dnas_rs_decode call (zeros with host != 0) */
} dnas_outer_stats;
int64_t dnas_outer_blocks(int64_t file_len, int32_t k, int32_t L);
uint8_t dnas_outer_crc8(const uint8_t *bytes, int64_t len);
int dnas_outer_frame(int64_t strand, const uint8_t *body, int32_t L, uint8_t *out_record);
int dnas_outer_encode(const uint8_t *file, int64_t file_len, int32_t n, int32_t k, int32_t L, int device_id, int host,
                      int64_t *out_n_blocks, uint8_t **out_records);
int dnas_outer_decode(int64_t n_records, const uint8_t *record_bytes, const int64_t *record_off, const double *weights, int32_t n,
                      int32_t k, int32_t L, int64_t B, int device_id, int host, uint8_t **out_data, int64_t *out_len,
                      int32_t *out_status, uint8_t *out_present, uint8_t *out_column_status, int32_t *out_fixed,
                      int64_t **out_failed_ranges, int64_t *out_n_ranges, dnas_outer_stats *out_stats);

/* The JSON the reference prints for --fit-error (MutatorParams::writeJSON, mutator.cpp:6-16) and
 * --error-counts (MutatorCounts::writeJSON, mutator.cpp:108-124), NUL-terminated into buf. */
int dnas_mutator_params_json(const dnas_mutator_params *p, char *buf, size_t cap);
int dnas_mutator_counts_json(const double *counts, int32_t n_len, char *buf, size_t cap);

/* ---- convenience: the whole reference call ------------------------------------------ */

typedef struct dnas_decoded dnas_decoded; /* vguard<FastSeq> result of decodeFastSeqs */
/* decodeFastSeqs(filename, machine, params) (viterbi.cpp:306-320) on GPU `device_id`; device_id = -1: on every GPU of
 * the node -- the reads of the file are dealt over the devices (by length, snake order), one host thread and one
 * model per device, results in file order: the serial loop of viterbi.cpp:312-318 has no dependence between reads.
 * dnas_decode_fastseqs_ex with want_events != 0 also keeps what the traceback found (the reference's level-3 log
 * messages, viterbi.cpp:266-293): per read a list of 64-bit events in the order the traceback met them,
 * type << 62 | position << 32 | payload -- 1: substitution at position, payload = emitted base << 2 | read base;
 * 2: deletion between position-1 and position, payload = the deleted base; 3: duplication at position, payload =
 * count << 26 | the duplicated bases, 2 bits each, first one in the highest bits (a model with more than 13 duplication
 * lanes cannot log them: dnas_model_set_event_log then returns DNAS_E_UNSUPPORTED). */
int dnas_decode_fastseqs(const char *fasta_path, const dnas_machine *m, const dnas_mutator_params *p,
                         int device_id, dnas_decoded **out);
int dnas_decode_fastseqs_ex(const char *fasta_path, const dnas_machine *m, const dnas_mutator_params *p,
                            int device_id, int want_events, dnas_decoded **out);
/* The same with a strand mode (DNAS_STRAND_*, see dnas_viterbi_batch_strands); dnas_decoded_strand: 1 when read i was
 * decoded from its reverse complement (its events then count positions along the reverse-complemented read), else 0.
 * device_id = -1 deals the reads of the file, not their orientations: both lattices of a read are filled on one device. */
int dnas_decode_fastseqs_strands(const char *fasta_path, const dnas_machine *m, const dnas_mutator_params *p,
                                 int device_id, int want_events, int strand_mode, dnas_decoded **out);
int dnas_decoded_strand(const dnas_decoded *d, int64_t i);
const char *dnas_decoded_tier(const dnas_decoded *d);   /* which fill kernel served the machine ("tier A: ...") */
int dnas_decoded_devices(const dnas_decoded *d);         /* how many devices shared the reads */
int64_t dnas_decoded_events(const dnas_decoded *d, int64_t i, const uint64_t **events);
/* GPUs visible to the library. */
int dnas_device_count(void);
int64_t dnas_decoded_count(const dnas_decoded *d);
const char *dnas_decoded_name(const dnas_decoded *d, int64_t i);
const char *dnas_decoded_seq(const dnas_decoded *d, int64_t i);
double dnas_decoded_loglike(const dnas_decoded *d, int64_t i);
void dnas_decoded_free(dnas_decoded *d);

/* FASTA/FASTQ(.gz) reader, readFastSeqs (fastseq.cpp:123-148): names + sequences. */
typedef struct dnas_fastseqs dnas_fastseqs;
int dnas_fastseqs_read(const char *path, dnas_fastseqs **out);
int64_t dnas_fastseqs_count(const dnas_fastseqs *f);
const char *dnas_fastseqs_name(const dnas_fastseqs *f, int64_t i);
const char *dnas_fastseqs_seq(const dnas_fastseqs *f, int64_t i);
void dnas_fastseqs_free(dnas_fastseqs *f);

const char *dnas_last_error(void);
void dnas_free(void *p);
/* 1 when the library was built with its HIP kernels (always, for the shipped .so). */
int dnas_has_device_code(void);
/* A testing aid.  With DNAS_DEBUG_ALLOC=<byte> in the environment (decimal or 0x.., 0 to 255; read at each allocation) every
 * device and pinned allocation of the library is filled with that byte and followed by a guard band of 256 bytes of it, which the
 * block's free compares.  out: guarded allocations made, guarded frees checked, guard violations (blocks whose band had changed),
 * the bytes of the first violated allocation, the offset of its first changed guard byte.  reset != 0: the counters start again
 * at 0.  The first violation also prints one line on stderr. */
int dnas_debug_alloc_stats(int64_t out[5], int reset);

#ifdef __cplusplus
}
#endif
#endif /* DNASTORE_AMD_H */
