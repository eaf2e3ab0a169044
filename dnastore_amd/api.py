"""Python mirror of the reference's interface for the Viterbi path, over the C ABI.

Same names and argument meaning as the reference: Machine.fromFile (trans.cpp:477-482),
MutatorParams from CLI flags (t/dnastore.cpp:119-129) or --error-file JSON
(mutator.cpp:18-49), decodeFastSeqs(filename, machine, params) (viterbi.cpp:306-320),
ViterbiMatrix.traceback()/loglike() (viterbi.h:94-102) batched as ViterbiDecoder.decode.
All computation happens in libdnastore_amd.so; nothing here touches the DP.
"""
import ctypes

import numpy as np

from . import lib as _l


class Machine:
    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def fromFile(path):
        h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_machine_load_json(str(path).encode(), ctypes.byref(h)))
        return Machine(h)

    @staticmethod
    def fromJSON(text):
        b = text.encode() if isinstance(text, str) else text
        h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_machine_parse_json(b, len(b), ctypes.byref(h)))
        return Machine(h)

    def nStates(self):
        return _l.lib().dnas_machine_n_states(self._h)

    def toJSON(self):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _l.check(_l.lib().dnas_machine_write_json(self._h, ctypes.byref(p), ctypes.byref(n)))
        s = ctypes.string_at(p, n.value).decode()
        _l.lib().dnas_free(p)
        return s

    def _encode(self, fn, data):
        p, n = ctypes.c_void_p(), ctypes.c_size_t()
        _l.check(fn(self._h, data, len(data), ctypes.byref(p), ctypes.byref(n)))
        s = ctypes.string_at(p, n.value).decode()
        _l.lib().dnas_free(p)
        return s

    @staticmethod
    def compose(first, second):
        """Machine::compose(first, second) (trans.cpp:505-602)."""
        h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_machine_compose(first._h, second._h, ctypes.byref(h)))
        return Machine(h)

    def decodeExact(self, dna):
        """Decoder<ostream>::decodeString + close (decoder.h:123-190): DNA -> symbol string."""
        return self._encode(_l.lib().dnas_decode_exact, dna.encode() if isinstance(dna, str) else dna)

    def encodeSymbols(self, symbols):
        """Encoder::encodeSymbolString + close (encoder.h:33-57,238-241) -> DNA string."""
        return self._encode(_l.lib().dnas_encode_symbols, symbols.encode() if isinstance(symbols, str) else symbols)

    def encodeBytes(self, payload):
        """Encoder::encodeString/encodeStream (encoder.h:222-237): bits LSB first -> DNA string."""
        return self._encode(_l.lib().dnas_encode_bytes, bytes(payload))

    def __del__(self):
        try:      # (at interpreter shutdown the module globals may be gone already)
            if getattr(self, "_h", None) is not None and self._h.value:
                _l.lib().dnas_machine_free(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


class MutatorParams:
    def __init__(self, c):
        self.c = c

    @staticmethod
    def fromFlags(sub=.01, iv=10., dup=.001, del_open=.001, del_ext=.01, global_=False, length=12):
        """--error-sub-prob/--error-iv-ratio/--error-dup-prob/--error-del-open/--error-del-ext/--error-global/--length."""
        c = _l.MutatorParamsC()
        _l.check(_l.lib().dnas_mutator_params_from_flags(sub, iv, dup, del_open, del_ext, int(bool(global_)), int(length),
                                                         ctypes.byref(c)))
        return MutatorParams(c)

    @staticmethod
    def fromFile(path):
        c = _l.MutatorParamsC()
        _l.check(_l.lib().dnas_mutator_params_load_json(str(path).encode(), ctypes.byref(c)))
        return MutatorParams(c)

    @property
    def local(self):
        return bool(self.c.local)

    @property
    def pLen(self):
        return [self.c.p_len[i] for i in range(self.c.n_len)]


_BASE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate("ACGT"):
    _BASE[ord(_ch)] = _i
    _BASE[ord(_ch.lower())] = _i


def tokenize(seq):
    """FastSeq::tokens over ACGT, case-insensitive (fastseq.cpp:9-39); raises on any other character."""
    b = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    t = _BASE[b]
    if (t == 255).any():
        bad = chr(int(b[np.argmax(t == 255)]))
        raise ValueError("Unknown symbol %s in sequence (alphabet is ACGT)" % bad)
    return t


def reverse_complement(seq):
    """The other strand of a read: str (ACGT, any case) -> str in upper case; an array of base codes 0..3 -> uint8 array
    (dnas_reverse_complement: 3 - code, order reversed)."""
    t = tokenize(seq) if isinstance(seq, (str, bytes)) else np.ascontiguousarray(seq, dtype=np.uint8)
    out = np.zeros(max(len(t), 1), dtype=np.uint8)
    t = np.ascontiguousarray(t)
    _l.check(_l.lib().dnas_reverse_complement(t.ctypes.data if len(t) else None, len(t), out.ctypes.data))
    out = out[:len(t)]
    return "".join("ACGT"[b] for b in out) if isinstance(seq, (str, bytes)) else out


class FlatModel:
    """MachineScores + InputModel + MutatorScores as flat arrays (dnas_flatten)."""

    def __init__(self, machine, params):
        self._h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_flatten(machine._h, ctypes.byref(params.c), ctypes.byref(self._h)))
        self.view = _l.lib().dnas_flat_view(self._h)

    def arrays(self):
        v = self.view.contents
        n, ne, nn, d = v.n_states, v.n_emit, v.n_null, max(1, v.max_dup_len)

        def arr(p, k, dt):
            return np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt).copy()
        return dict(
            n_states=n, max_dup_len=v.max_dup_len, n_len=v.n_len, local=v.local, n_emit=ne, n_null=nn,
            ein_ptr=arr(v.ein_ptr, n + 1, np.int32), ein_src=arr(v.ein_src, ne, np.int32),
            ein_score=arr(v.ein_score, ne, np.float64), ein_in=arr(v.ein_in, ne, np.uint8),
            ein_base=arr(v.ein_base, ne, np.uint8),
            nin_ptr=arr(v.nin_ptr, n + 1, np.int32), nin_src=arr(v.nin_src, nn, np.int32),
            nin_score=arr(v.nin_score, nn, np.float64), nin_in=arr(v.nin_in, nn, np.uint8),
            eout_ptr=arr(v.eout_ptr, n + 1, np.int32), eout_dst=arr(v.eout_dst, ne, np.int32),
            nout_ptr=arr(v.nout_ptr, n + 1, np.int32), nout_dst=arr(v.nout_dst, nn, np.int32),
            mdl=arr(v.mdl, n, np.uint8), ctx=arr(v.ctx, n * d, np.uint8).reshape(n, d), topo=arr(v.topo, n, np.int32),
            scores=np.array([v.del_open, v.tan_dup, v.no_gap, v.del_extend, v.del_end] + list(v.sub)
                            + [v.len[i] for i in range(v.n_len)]),
            alphabet=v.alphabet.decode(), sym_logp=np.array(list(v.sym_logp)))

    def plan_slots(self):
        """Tier-A placement: (lds_index int32[N] = row*T + lane, lattice_slot int32[N], T, K)."""
        n = self.view.contents.n_states
        lds = np.full(n, -1, dtype=np.int32)
        lat = np.full(n, -1, dtype=np.int32)
        t, k = ctypes.c_int32(), ctypes.c_int32()
        _l.check(_l.lib().dnas_tiera_plan_slots(self.view, lds.ctypes.data, lat.ctypes.data, ctypes.addressof(t), ctypes.addressof(k)))
        return lds, lat, t.value, k.value

    def plan_tables(self):
        """Tier-A tables as the fill kernel receives them: (row_shapes int32[K][2], entries uint32[nEntries][T],
        meta uint32[K][T], n_s_rows)."""
        _, _, t, k = self.plan_slots()
        ne, ns = ctypes.c_int32(), ctypes.c_int32()
        _l.check(_l.lib().dnas_tiera_plan_tables(self.view, None, None, 0, None, ctypes.addressof(ne), ctypes.addressof(ns)))
        shapes = np.zeros((k, 2), dtype=np.int32)
        ent = np.zeros((ne.value, t), dtype=np.uint32)
        meta = np.zeros((k, t), dtype=np.uint32)
        _l.check(_l.lib().dnas_tiera_plan_tables(self.view, shapes.ctypes.data, ent.ctypes.data, ent.size, meta.ctypes.data,
                                                 ctypes.addressof(ne), ctypes.addressof(ns)))
        return shapes, ent, meta, ns.value

    def cluster_plan(self, members=0):
        """Tier-C tables (members = 1: the tier-A plan): dict(G, K, T, n_entries, n_s_rows, n_inbox_rows, shapes int32[K][6],
        entries uint32[G][n_entries][T], meta uint32[G][K][T], member_of, lds_index, lattice_slot, fold uint32[G][n_inbox_rows][T],
        proxy_member, proxy_lds_index: the places of the plan's proxies)."""
        n = self.view.contents.n_states
        info = np.zeros(8, dtype=np.int32)
        _l.check(_l.lib().dnas_tierc_plan(self.view, int(members), info.ctypes.data, None, None, 0, None, None, None, None, None))
        G, K, T, ne = (int(v) for v in info[:4])
        shapes = np.zeros((K, 6), dtype=np.int32)
        fold = np.zeros((G, max(int(info[5]), 1), T), dtype=np.uint32)
        ent = np.zeros((G, ne, T), dtype=np.uint32)
        meta = np.zeros((G, K, T), dtype=np.uint32)
        member_of = np.full(n, -1, dtype=np.int32)
        lds = np.full(n, -1, dtype=np.int32)
        lat = np.full(n, -1, dtype=np.int32)
        _l.check(_l.lib().dnas_tierc_plan(self.view, G, info.ctypes.data, shapes.ctypes.data, ent.ctypes.data, ent.size, meta.ctypes.data,
                                          member_of.ctypes.data, lds.ctypes.data, lat.ctypes.data, fold.ctypes.data))
        n_prox = int(info[6])
        pm = np.zeros(max(n_prox, 1), dtype=np.int32)
        pl = np.zeros(max(n_prox, 1), dtype=np.int32)
        if n_prox:
            _l.check(_l.lib().dnas_tierc_plan_proxies(self.view, G, pm.ctypes.data, pl.ctypes.data, n_prox))
        out = dict(G=G, K=K, T=T, n_entries=ne, n_s_rows=int(info[4]), n_inbox_rows=int(info[5]), shapes=shapes, entries=ent, meta=meta,
                   member_of=member_of, lds_index=lds, lattice_slot=lat, fold=fold[:, :int(info[5])],
                   proxy_member=pm[:n_prox], proxy_lds_index=pl[:n_prox])
        return out

    def tune_record_name(self, members=1, threads=0):
        """File name of this machine's row-program tuning record (kernel cache / dnastore_amd/tune/): members = 1 as tier A,
        0 / >= 2 as tier C with the smallest / that cluster."""
        buf = ctypes.create_string_buffer(64)
        _l.check(_l.lib().dnas_tune_record_name(self.view, int(members), int(threads), buf, 64))
        return buf.value.decode()

    @staticmethod
    def kernel_source_hash():
        """Hash of the fill kernel's source inside the library (what tuning records name as kernel=)."""
        buf = ctypes.create_string_buffer(32)
        _l.check(_l.lib().dnas_kernel_source_hash(buf, 32))
        return buf.value.decode()

    def precompile_cluster(self, members=0):
        """JIT-specialise the cluster (tier C) fill kernel for this machine into the kernel cache (no GPU needed)."""
        buf = ctypes.create_string_buffer(4096)
        _l.check(_l.lib().dnas_tierc_precompile(self.view, int(members), buf, 4096))
        return buf.value.decode()

    def precompile(self):
        """JIT-specialise the tier-A fill kernel for this machine into dnastore_amd/kcache (no GPU needed)."""
        buf = ctypes.create_string_buffer(1024)
        _l.check(_l.lib().dnas_tiera_precompile(self.view, buf, 1024))
        return buf.value.decode()

    def __del__(self):
        try:      # (at interpreter shutdown the module globals may be gone already)
            if getattr(self, "_h", None) is not None and self._h.value:
                _l.lib().dnas_flat_free(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


def slot_needed(sym, out_offsets, i):
    """dnas_slot_needed: the length read i, status DNAS_READ_OUT_OVERFLOW, left at the front of its slot of the host buffer sym."""
    at, cap = int(out_offsets[i]), int(out_offsets[i + 1]) - int(out_offsets[i])
    return int.from_bytes(sym[at:at + 8].tobytes(), "little") if cap >= 8 else 0


class _SlotsTooSmall(Exception):
    """A call in slots the front end sized itself left a string overflowed; .caps: per slot array, the slots to call again with."""

    def __init__(self, caps):
        super().__init__("slots too small")
        self.caps = caps

    @staticmethod
    def check(*arrays):
        """arrays: (sym, out_offsets, status) per slot array of a call.  Raises if a status is DNAS_READ_OUT_OVERFLOW."""
        caps, grown = [], False
        for sym, ooff, st in arrays:
            c = np.diff(ooff).astype(np.int64)
            for i in np.flatnonzero(st == _l.READ_OUT_OVERFLOW):
                need = slot_needed(sym, ooff, i)
                if need <= c[i]:
                    raise _l.DnasError(-7, "a read overflowed its slot and left no longer length behind")
                c[i], grown = need, True
            caps.append(c)
        if grown:
            raise _SlotsTooSmall(tuple(caps) if len(caps) > 1 else (caps[0], None))


def pack_reads(reads):
    """list of str -> (read_offsets uint64[n+1], bases uint8[total]) as the C ABI wants them."""
    toks = [tokenize(r) for r in reads]
    off = np.zeros(len(toks) + 1, dtype=np.uint64)
    if toks:
        off[1:] = np.cumsum([len(t) for t in toks])
    bases = np.concatenate(toks).astype(np.uint8) if toks and off[-1] else np.zeros(1, np.uint8)
    return off, bases


class ViterbiDecoder:
    """A (machine, params) pair resident on one GPU; decode() is the batched ViterbiMatrix + traceback."""

    def __init__(self, machine, params, device=0, arena_bytes=0, options=None):
        """options: dnas_model_create_ex's "key=value,..." string, e.g. "tier=C,cluster=2"."""
        self.machine, self.params = machine, params
        self.flat = FlatModel(machine, params)
        v = self.flat.view.contents
        self.n_states, self.max_dup_len = v.n_states, v.max_dup_len
        self._h = ctypes.c_void_p()
        self._event_log = False
        _l.check(_l.lib().dnas_model_create_ex(self.flat.view, int(device), int(arena_bytes),
                                               options.encode() if options else None, ctypes.byref(self._h)))

    def _batch(self, off, bases, caps, mode):
        """dnas_viterbi_batch (mode forward) / dnas_viterbi_batch_strands on packed host arrays, read i in a slot of caps[i] symbols
        -> (sym, out_offsets, out_len, loglike, status, strand or None)."""
        n = len(off) - 1
        ooff = np.zeros(n + 1, dtype=np.uint64)
        if n:
            ooff[1:] = np.cumsum(caps)
        sym = np.empty(max(int(ooff[-1]), 1), dtype=np.uint8)
        olen = np.zeros(max(n, 1), dtype=np.uint32)
        ll = np.zeros(max(n, 1), dtype=np.float64)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        if mode != _l.STRAND_FORWARD:
            strand = np.zeros(max(n, 1), dtype=np.uint8)
            _l.check(_l.lib().dnas_viterbi_batch_strands(self._h, n, off.ctypes.data, bases.ctypes.data, mode, sym.ctypes.data,
                                                         ooff.ctypes.data, olen.ctypes.data, ll.ctypes.data, st.ctypes.data,
                                                         strand.ctypes.data))
            return sym, ooff, olen[:n], ll[:n], st[:n], strand[:n]
        _l.check(_l.lib().dnas_viterbi_batch(self._h, n, off.ctypes.data, bases.ctypes.data, sym.ctypes.data,
                                             ooff.ctypes.data, olen.ctypes.data, ll.ctypes.data, st.ctypes.data))
        return sym, ooff, olen[:n], ll[:n], st[:n], None

    def _batch_own_slots(self, off, bases, mode):
        """_batch in slots this front end sizes itself: 4 L + 64 symbols for a read of L bases, which is a guess -- a walk decodes
        a symbol for every state it passes, with or without a base of the read.  A read that overflowed its slot left there the
        length it needs (include/dnastore_amd.h); those reads, and only they, are decoded once more in slots of that size, and the
        results are laid out as one call's.  A call without one returns what the one call gave."""
        off = np.ascontiguousarray(off, dtype=np.uint64)
        caps = 4 * np.diff(off).astype(np.int64) + 64
        sym, ooff, olen, ll, st, strand = self._batch(off, bases, caps, mode)
        over = np.flatnonzero(st == _l.READ_OUT_OVERFLOW)
        if not len(over):
            return sym, ooff, olen, ll, st, strand
        need = np.array([slot_needed(sym, ooff, i) for i in over], dtype=np.int64)
        if (need <= caps[over]).any():
            raise _l.DnasError(-7, "a read overflowed its slot and left no longer length behind")
        if self._event_log:                # dnas_model_read_events counts in the last call's reads: that call is the whole batch
            caps[over] = need
            return self._batch(off, bases, caps, mode)
        sub_off = np.zeros(len(over) + 1, dtype=np.uint64)
        sub_off[1:] = np.cumsum(np.diff(off)[over])
        parts = [bases[int(off[i]):int(off[i + 1])] for i in over]
        sub_bases = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint8) if int(sub_off[-1]) else np.zeros(1, np.uint8)
        sub = self._batch(sub_off, sub_bases, need, mode)
        caps[over] = need
        all_off = np.zeros(len(caps) + 1, dtype=np.uint64)
        all_off[1:] = np.cumsum(caps)
        out = np.empty(max(int(all_off[-1]), 1), dtype=np.uint8)
        for i in range(len(caps)):
            out[int(all_off[i]):int(all_off[i]) + int(olen[i])] = sym[int(ooff[i]):int(ooff[i]) + int(olen[i])]
        for j, i in enumerate(over):
            out[int(all_off[i]):int(all_off[i]) + int(sub[2][j])] = sub[0][int(sub[1][j]):int(sub[1][j]) + int(sub[2][j])]
            olen[i], ll[i], st[i] = sub[2][j], sub[3][j], sub[4][j]
            if strand is not None:
                strand[i] = sub[5][j]
        return out, all_off, olen, ll, st, strand

    def decode(self, reads, out_cap=None, strands="forward"):
        """reads: list of str (ACGT, any case) -> (decoded symbol strings, loglike float64[n], status uint8[n]).
        out_cap=None: the slots are the front end's own and every string is delivered, however long (_batch_own_slots);
        out_cap=k: every read gets a slot of k symbols, and a longer string is status 2 (DNAS_READ_OUT_OVERFLOW) and "".
        strands="reverse": every read is decoded as its reverse complement; "both": each read as written and reverse-complemented,
        the orientation with the strictly larger log-likelihood kept (ties: forward) -- the tuple then ends with the strand
        array uint8[n], 1 = decoded from the reverse complement (dnas_viterbi_batch_strands)."""
        mode = _l.strand_mode(strands)
        off, bases = pack_reads(reads)
        got = self.decode_packed(off, bases, out_cap=out_cap, strands=mode)
        sym, ooff, olen = got[:3]
        out = [sym[int(ooff[i]):int(ooff[i]) + int(olen[i])].tobytes().decode() for i in range(len(reads))]
        return (out,) + tuple(got[3:])

    def _with_support(self, out, reads, clusters, band):
        """decode_clusters(..., support=True): one pairProfiles call on this decoder's GPU over (winning strand, read) for every
        read of every cluster that has a winner, the reads oriented by the per-read strand flags."""
        members = {}
        for i, lab in enumerate(clusters):
            members.setdefault(lab, []).append(i)
        strands, ins, outs, flags, owner = [], [], [], [], []
        for c, lab in enumerate(out.labels):
            won = out.read[c] >= 0 or out.source[c] == 1
            strands.append(_tokens(self.machine.encodeSymbols(out.symbols[c])) if won else np.zeros(0, dtype=np.int8))
            for i in (members[lab] if won else []):
                ins.append(strands[c])
                outs.append(reads[i])
                flags.append(int(out.per_read[3][i]))
                owner.append(c)
        prof = pairProfiles(self.params, ins, outs, band=band, read_strand=flags, device=_l.lib().dnas_model_device(self._h))
        out.support = [np.zeros(len(s)) for s in strands]
        out.support_reads = np.zeros(len(out.labels), dtype=np.int64)
        for j, c in enumerate(owner):
            if prof.status[j] == _l.COUNTS_OK:
                s = strands[c]
                out.support[c] += prof.pair_profiles[j][_l.PROFILE_MATCH + s, np.arange(len(s))]
                out.support_reads[c] += 1
        for c, v in enumerate(out.support_reads):
            if v:
                out.support[c] /= v
        return out

    def decode_clusters(self, reads, clusters, strands="both", band=32, polish=0, score="viterbi", support=False):
        """dnas_viterbi_clusters: one message per cluster of reads.  clusters: one label per read; the reads are grouped by label
        in order of the labels' first appearance, their order kept inside a cluster.  Every read is decoded (strands as for
        decode), each cluster's candidates are the distinct strands its reads' messages encode to, and the winner is the
        candidate with the largest joint pair-HMM score over all reads of the cluster (consensusScore, band as there).
        polish=N > 0 (dnas_viterbi_clusters_ex): the cluster's first read, polished by all its reads for at most N rounds
        (consensusReads), is decoded too, and its message is one more candidate.  score="forward"
        (dnas_viterbi_clusters_scored): the candidates are compared by the reads' marginal likelihood (pairLikelihoods) instead of
        their best alignment's score, and the result has .confidence, the winner's posterior per cluster.  support=True: which
        bases of the winning strand the reads back -- .support[c] float64[I_c], the posterior that base r of cluster c's winning
        strand (machine.encodeSymbols of its message) was read as itself, averaged over the .support_reads[c] reads of the
        cluster that have a path to it inside the band (pairProfiles); an empty array for a cluster without a winner.
        -> ClusterDecodes."""
        if support:
            out = self.decode_clusters(reads, clusters, strands=strands, band=band, polish=polish, score=score)
            return self._with_support(out, reads, clusters, band)
        try:
            return self._decode_clusters_once(reads, clusters, strands, band, polish, score, None)
        except _SlotsTooSmall as e:        # the front end's own slots were a guess: once more, with the lengths the reads left
            return self._decode_clusters_once(reads, clusters, strands, band, polish, score, e.caps)

    def _decode_clusters_once(self, reads, clusters, strands, band, polish, score, caps):
        """decode_clusters with the reads (and, polish > 0, the consensus reads) in slots of caps = (per read in grouped order, per
        cluster); None: 4 L + 64 symbols for L bases, and _SlotsTooSmall with the slots to use if a string overflowed one."""
        smode = _l.score_mode(score)
        if len(clusters) != len(reads):
            raise ValueError("%d cluster labels for %d reads" % (len(clusters), len(reads)))
        mode = _l.strand_mode(strands)
        labels, members = [], {}
        for i, lab in enumerate(clusters):
            if lab not in members:
                members[lab] = []
                labels.append(lab)
            members[lab].append(i)
        order = [i for lab in labels for i in members[lab]]
        n, nc = len(order), len(labels)
        cl_off = np.zeros(nc + 1, dtype=np.int64)
        if nc:
            cl_off[1:] = np.cumsum([len(members[lab]) for lab in labels])
        off, bases = pack_reads([reads[i] for i in order])
        ooff = np.zeros(n + 1, dtype=np.uint64)
        if n:
            ooff[1:] = np.cumsum(4 * np.diff(off).astype(np.int64) + 64 if caps is None else caps[0])
        sym = np.zeros(max(int(ooff[-1]), 1), dtype=np.uint8)
        olen = np.zeros(max(n, 1), dtype=np.uint32)
        ll = np.zeros(max(n, 1), dtype=np.float64)
        st, strand = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
        read = np.zeros(max(nc, 1), dtype=np.int64)
        total, second = np.zeros(max(nc, 1)), np.zeros(max(nc, 1))
        ncand, votes = np.zeros(max(nc, 1), dtype=np.int32), np.zeros(max(nc, 1), dtype=np.int32)
        status = np.zeros(max(nc, 1), dtype=np.uint8)
        cs = _l.ConsensusStatsC()
        if polish:
            return self._decode_clusters_ex(int(polish), int(band), mode, labels, order, n, nc, cl_off, off, bases, ooff, sym, olen, ll, st,
                                            strand, read, total, second, ncand, votes, status, cs, smode, caps)
        conf = None
        if smode != _l.SCORE_VITERBI:
            conf = np.zeros(max(nc, 1))
            _l.check(_l.lib().dnas_viterbi_clusters_scored(self._h, self.machine._h, ctypes.byref(self.params.c), int(band), n,
                                                           off.ctypes.data, bases.ctypes.data, cl_off.ctypes.data, nc, mode, 0,
                                                           sym.ctypes.data, ooff.ctypes.data, olen.ctypes.data, ll.ctypes.data,
                                                           st.ctypes.data, strand.ctypes.data, read.ctypes.data, total.ctypes.data,
                                                           second.ctypes.data, ncand.ctypes.data, votes.ctypes.data, status.ctypes.data,
                                                           None, None, None, None, None, None, None, None, smode, conf.ctypes.data,
                                                           ctypes.byref(cs)))
        else:
            _l.check(_l.lib().dnas_viterbi_clusters(self._h, self.machine._h, ctypes.byref(self.params.c), int(band), n,
                                                    off.ctypes.data, bases.ctypes.data, cl_off.ctypes.data, nc, mode, sym.ctypes.data,
                                                    ooff.ctypes.data,
                                                    olen.ctypes.data, ll.ctypes.data, st.ctypes.data, strand.ctypes.data,
                                                    read.ctypes.data, total.ctypes.data, second.ctypes.data, ncand.ctypes.data,
                                                    votes.ctypes.data, status.ctypes.data, ctypes.byref(cs)))
        if caps is None:
            _SlotsTooSmall.check((sym, ooff, st[:n]))
        text = [sym[int(ooff[k]):int(ooff[k]) + int(olen[k])].tobytes().decode() for k in range(n)]
        back = np.argsort(np.array(order, dtype=np.int64), kind="stable") if n else np.zeros(0, np.int64)   # grouped position of read i
        per_read = ([text[k] for k in back], ll[:n][back], st[:n][back], strand[:n][back])
        symbols = [text[int(r)] if r >= 0 else "" for r in read[:nc]]
        orig = np.array([order[int(r)] if r >= 0 else -1 for r in read[:nc]], dtype=np.int64)
        out = ClusterDecodes(labels, symbols, orig, total[:nc], second[:nc], votes[:nc], ncand[:nc], status[:nc], per_read,
                             {k: getattr(cs, k) for k, _ in cs._fields_})
        if conf is not None:
            out.confidence = conf[:nc]
        return out

    def _decode_clusters_ex(self, polish, band, mode, labels, order, n, nc, cl_off, off, bases, ooff, sym, olen, ll, st, strand, read,
                            total, second, ncand, votes, status, cs, smode=0, caps=None):
        lens = np.diff(off).astype(np.int64)
        # a consensus read is at most `polish` x 2 x the cluster's longest read longer than the first read
        grow = [int(lens[cl_off[c]]) + 2 * polish * int(lens[cl_off[c]:cl_off[c + 1]].max()) if cl_off[c + 1] > cl_off[c] else 0
                for c in range(nc)]
        coff = np.zeros(nc + 1, dtype=np.uint64)
        if nc:
            coff[1:] = np.cumsum(4 * np.array(grow, dtype=np.int64) + 64 if caps is None else caps[1])
        csym = np.zeros(max(int(coff[-1]), 1), dtype=np.uint8)
        clen = np.zeros(max(nc, 1), dtype=np.uint32)
        cll = np.zeros(max(nc, 1), dtype=np.float64)
        cst, source = np.zeros(max(nc, 1), dtype=np.uint8), np.zeros(max(nc, 1), dtype=np.uint8)
        cons, cons_off = ctypes.c_void_p(), np.zeros(nc + 1, dtype=np.int64)
        head = [self._h, self.machine._h, ctypes.byref(self.params.c), band, n, off.ctypes.data, bases.ctypes.data, cl_off.ctypes.data, nc,
                mode, polish, sym.ctypes.data, ooff.ctypes.data, olen.ctypes.data, ll.ctypes.data, st.ctypes.data, strand.ctypes.data,
                read.ctypes.data, total.ctypes.data, second.ctypes.data, ncand.ctypes.data, votes.ctypes.data, status.ctypes.data,
                source.ctypes.data, ctypes.byref(cons), cons_off.ctypes.data, csym.ctypes.data, coff.ctypes.data, clen.ctypes.data,
                cll.ctypes.data, cst.ctypes.data]
        conf = None
        if smode != _l.SCORE_VITERBI:
            conf = np.zeros(max(nc, 1))
            _l.check(_l.lib().dnas_viterbi_clusters_scored(*head, smode, conf.ctypes.data, ctypes.byref(cs)))
        else:
            _l.check(_l.lib().dnas_viterbi_clusters_ex(*head, ctypes.byref(cs)))
        flat = _take(cons, ctypes.c_int8, int(cons_off[nc]), np.int8)
        if caps is None:
            _SlotsTooSmall.check((sym, ooff, st[:n]), (csym, coff, cst[:nc]))
        text = [sym[int(ooff[k]):int(ooff[k]) + int(olen[k])].tobytes().decode() for k in range(n)]
        ctext = [csym[int(coff[c]):int(coff[c]) + int(clen[c])].tobytes().decode() for c in range(nc)]
        back = np.argsort(np.array(order, dtype=np.int64), kind="stable") if n else np.zeros(0, np.int64)
        per_read = ([text[k] for k in back], ll[:n][back], st[:n][back], strand[:n][back])
        symbols = [ctext[c] if source[c] else (text[int(read[c])] if read[c] >= 0 else "") for c in range(nc)]
        orig = np.array([order[int(r)] if r >= 0 else -1 for r in read[:nc]], dtype=np.int64)
        out = ClusterDecodes(labels, symbols, orig, total[:nc], second[:nc], votes[:nc], ncand[:nc], status[:nc], per_read,
                             {k: getattr(cs, k) for k, _ in cs._fields_})
        out.source = source[:nc]
        out.consensus_reads = ["".join("ACGT"[b] for b in flat[int(cons_off[c]):int(cons_off[c + 1])]) for c in range(nc)]
        out.consensus_decodes = (ctext, cll[:nc], cst[:nc])
        if conf is not None:
            out.confidence = conf[:nc]
        with np.errstate(invalid="ignore"):
            out.margin = np.where((out.read >= 0) | (out.source == 1), out.total - out.second, -np.inf)
        return out

    def decode_pool(self, reads, strands="both", band=32, polish=0, score="viterbi", support=False, primers=None, **cluster_options):
        """A pool of reads of unknown origin and orientation -> one message per strand it holds: clusterReads(self.params, reads,
        band=band, **cluster_options) on this decoder's GPU forms the clusters, decode_clusters decodes them (polish, score and
        support as there).
        -> ClusterDecodes, its labels the cluster ids; .clusters is the ReadClusters.
        primers (a list of (F, R), as trimReads takes them): the reads are raw -- primers and junk around the payload.  They are
        trimmed first on this decoder's GPU, the options whose names begin with trim_ going to trimReads (trim_max_offset,
        trim_max_edit_permille, trim_anchors, trim_min_payload) and to TrimmedReads.kept (trim_pair, trim_min_margin), and the
        kept payloads are the pool.  .read then counts in the caller's reads; .kept int64[n] names the caller's read behind each
        payload, the order .per_read and .clusters follow; .trimmed is the TrimmedReads."""
        if primers is not None:
            trim = {k[5:]: cluster_options.pop(k) for k in list(cluster_options) if k.startswith("trim_")}
            keep = {k: trim.pop(k) for k in ("pair", "min_margin") if k in trim}
            trim.setdefault("device", _l.lib().dnas_model_device(self._h))
            trimmed = trimReads(primers, reads, **trim)
            kept = np.array(trimmed.kept(**keep), dtype=np.int64)
            payloads = trimmed.payloads()
            out = self.decode_pool(["".join("ACGT"[b] for b in _tokens(payloads[i])) for i in kept], strands=strands, band=band, polish=polish, score=score, support=support,
                                   **cluster_options)
            out.read = np.array([kept[r] if r >= 0 else -1 for r in out.read], dtype=np.int64)
            out.kept, out.trimmed = kept, trimmed
            return out
        cluster_options.setdefault("device", _l.lib().dnas_model_device(self._h))
        found = clusterReads(self.params, reads, band=band, **cluster_options)
        out = self.decode_clusters(reads, found.labels(), strands=strands, band=band, polish=polish, score=score, support=support)
        out.clusters = found
        return out

    def decode_packed(self, read_offsets, bases, out_cap=None, strands="forward"):
        """dnas_viterbi_batch on packed HOST arrays (pack_reads' layout), results as arrays: (sym uint8[...], out_offsets uint64[n+1],
        out_len uint32[n], loglike float64[n], status uint8[n]) -- the call a C caller makes: bases in over PCIe, strings out.
        strands other than "forward" (see decode): dnas_viterbi_batch_strands, the tuple ends with strand uint8[n]."""
        mode = _l.strand_mode(strands)
        if out_cap is None:
            got = self._batch_own_slots(read_offsets, bases, mode)
        else:
            got = self._batch(read_offsets, bases, np.full(len(read_offsets) - 1, int(out_cap), dtype=np.int64), mode)
        return got if mode != _l.STRAND_FORWARD else got[:5]

    def decode_device(self, read_offsets, d_bases_ptr, d_sym_ptr, out_offsets, d_len_ptr, d_ll_ptr, d_status_ptr,
                      strands="forward", d_strand_ptr=None):
        """dnas_viterbi_batch_device: raw device pointers (ints), host offset arrays; asynchronous.  strands other than
        "forward" (see decode): dnas_viterbi_batch_strands_device, which also fills d_strand_ptr (uint8[n] on the device)."""
        n = len(read_offsets) - 1
        mode = _l.strand_mode(strands)
        if mode != _l.STRAND_FORWARD or d_strand_ptr is not None:
            _l.check(_l.lib().dnas_viterbi_batch_strands_device(self._h, n, read_offsets.ctypes.data, d_bases_ptr, mode, d_sym_ptr,
                                                                out_offsets.ctypes.data, d_len_ptr, d_ll_ptr, d_status_ptr,
                                                                d_strand_ptr))
            return
        _l.check(_l.lib().dnas_viterbi_batch_device(self._h, n, read_offsets.ctypes.data, d_bases_ptr, d_sym_ptr,
                                                    out_offsets.ctypes.data, d_len_ptr, d_ll_ptr, d_status_ptr))

    def sync(self):
        _l.check(_l.lib().dnas_model_sync(self._h))

    @property
    def tier(self):
        """'tier A: <shape>' or 'tier B: <reason>' -- which fill kernel serves this machine."""
        return _l.lib().dnas_model_tier(self._h).decode()

    def cluster_census(self):
        """Tier C, last call: (clusters that ran, clusters whose members sat on more than one XCD)."""
        c, s = ctypes.c_int32(), ctypes.c_int32()
        _l.check(_l.lib().dnas_model_cluster_census(self._h, ctypes.addressof(c), ctypes.addressof(s)))
        return c.value, s.value

    def stats(self):
        """dnas_model_last_stats, and under "arena_slices" what dnas_model_last_arena_slices says."""
        s = _l.BatchStatsC()
        _l.check(_l.lib().dnas_model_last_stats(self._h, ctypes.byref(s)))
        slices = ctypes.c_int64()
        _l.check(_l.lib().dnas_model_last_arena_slices(self._h, ctypes.byref(slices)))
        out = {k: getattr(s, k) for k, _ in s._fields_}
        out["arena_slices"] = slices.value
        return out

    def strand_stats(self):
        """dnas_model_last_strand_stats: what the last call did about strands (all zero after a forward call)."""
        s = _l.StrandStatsC()
        _l.check(_l.lib().dnas_model_last_strand_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def set_event_log(self, on):
        """dnas_model_set_event_log: keep the traceback's events of the calls that follow (or stop keeping them)."""
        _l.check(_l.lib().dnas_model_set_event_log(self._h, int(bool(on))))
        self._event_log = bool(on)

    def events(self, read_index):
        """dnas_model_read_events: the traceback events of one read of the last call, as the reference's log lines."""
        n = ctypes.c_int64()
        _l.check(_l.lib().dnas_model_read_events(self._h, int(read_index), None, 0, ctypes.addressof(n)))
        out = np.zeros(max(n.value, 1), dtype=np.uint64)
        _l.check(_l.lib().dnas_model_read_events(self._h, int(read_index), out.ctypes.data, n.value, ctypes.addressof(n)))
        return [format_event(int(e)) for e in out[:n.value]]

    def lattice(self, read_index, length):
        """Lattice of one read of the last decode() call: float64 [L+1][D+2][N] (lanes S, D, T1..TD)."""
        out = np.empty((length + 1, self.max_dup_len + 2, self.n_states), dtype=np.float64)
        _l.check(_l.lib().dnas_model_read_lattice(self._h, int(read_index), int(length), out.ctypes.data))
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _l.lib().dnas_model_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_fastseqs(path):
    """readFastSeqs (fastseq.cpp:123-148) -> [(name, seq)]."""
    h = ctypes.c_void_p()
    _l.check(_l.lib().dnas_fastseqs_read(str(path).encode(), ctypes.byref(h)))
    L = _l.lib()
    out = [(L.dnas_fastseqs_name(h, i).decode(), L.dnas_fastseqs_seq(h, i).decode())
           for i in range(L.dnas_fastseqs_count(h))]
    L.dnas_fastseqs_free(h)
    return out


def format_event(ev):
    """One traceback event as the reference's level-3 log line (viterbi.cpp:266-293)."""
    kind, pos, pay = ev >> 62, (ev >> 32) & 0x3fffffff, ev & 0xffffffff
    if kind == 1:
        return "Substitution at %d: %s -> %s" % (pos, "ACGT"[(pay >> 2) & 3], "ACGT"[pay & 3])
    if kind == 2:
        return "Deletion between %d and %d: %s" % (pos - 1, pos, "ACGT"[pay & 3])
    n = pay >> 26
    return "Duplication at %d: %s" % (pos, "".join("ACGT"[(pay >> (2 * (n - 1 - i))) & 3] for i in range(n)))


def decode_fastseqs(filename, machine, params, device=0, events=False, info=None, strands="forward"):
    """decodeFastSeqs(filename, machine, params) (viterbi.cpp:306-320) -> [(name, decoded symbols, loglike)]
    (with events=True: [(name, symbols, loglike, [event lines])]).  device=-1: every GPU of the node.
    info: an optional dict that receives the fill tier and the number of devices used.
    strands="reverse" | "both" (ViterbiDecoder.decode): dnas_decode_fastseqs_strands; info then also receives "strand", the
    list of 0 / 1 per read (1: decoded from its reverse complement, event positions counted along it)."""
    h = ctypes.c_void_p()
    mode = _l.strand_mode(strands)
    if mode != _l.STRAND_FORWARD:
        _l.check(_l.lib().dnas_decode_fastseqs_strands(str(filename).encode(), machine._h, ctypes.byref(params.c), int(device),
                                                       int(bool(events)), mode, ctypes.byref(h)))
    else:
        _l.check(_l.lib().dnas_decode_fastseqs_ex(str(filename).encode(), machine._h, ctypes.byref(params.c), int(device),
                                                  int(bool(events)), ctypes.byref(h)))
    L = _l.lib()
    out = []
    for i in range(L.dnas_decoded_count(h)):
        rec = (L.dnas_decoded_name(h, i).decode(), L.dnas_decoded_seq(h, i).decode(), L.dnas_decoded_loglike(h, i))
        if events:
            p = ctypes.c_void_p()
            n = L.dnas_decoded_events(h, i, ctypes.byref(p))
            evs = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_uint64)), shape=(n,)).copy() if n else []
            rec = rec + ([format_event(int(e)) for e in evs],)
        out.append(rec)
    if info is not None:
        info["tier"] = L.dnas_decoded_tier(h).decode()
        info["devices"] = L.dnas_decoded_devices(h)
        if mode != _l.STRAND_FORWARD:
            info["strand"] = [L.dnas_decoded_strand(h, i) for i in range(L.dnas_decoded_count(h))]
    L.dnas_decoded_free(h)
    return out


class StockholmDB:
    """readStockholmDatabase (stockholm.cpp:154-167) of two-row alignments, flattened for the E-step."""

    def __init__(self, path):
        self._h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_stockholm_read(str(path).encode(), ctypes.byref(self._h)))
        self.view = _l.lib().dnas_pairs_get(self._h).contents
        self.n = self.view.n_pairs

    def arrays(self):
        """numpy copies: ins, in_off, outs, out_off, cm_in, cm_in_off, cm_out, cm_out_off."""
        v, n = self.view, self.n

        def arr(ptr, count, dt):
            if count == 0:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(count,)).copy()
        in_off = arr(v.in_off, n + 1, np.int64)
        out_off = arr(v.out_off, n + 1, np.int64)
        ci_off = arr(v.cm_in_off, n + 1, np.int64)
        co_off = arr(v.cm_out_off, n + 1, np.int64)
        return dict(ins=arr(v.in_seqs, int(in_off[-1]), np.int8), in_off=in_off, outs=arr(v.out_seqs, int(out_off[-1]), np.int8),
                    out_off=out_off, cm_in=arr(v.cm_in, int(ci_off[-1]), np.int32), cm_in_off=ci_off,
                    cm_out=arr(v.cm_out, int(co_off[-1]), np.int32), cm_out_off=co_off, n=n)

    def __del__(self):
        try:      # (at interpreter shutdown the module globals may be gone already)
            if getattr(self, "_h", None) is not None and self._h.value:
                _l.lib().dnas_pairs_free(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


def _pair_ptrs(pk):
    keys = ("ins", "in_off", "outs", "out_off", "cm_in", "cm_in_off", "cm_out", "cm_out_off")
    dts = (np.int8, np.int64, np.int8, np.int64, np.int32, np.int64, np.int32, np.int64)
    keep = [np.ascontiguousarray(pk[k], dtype=d) if len(pk[k]) else np.zeros(1, d) for k, d in zip(keys, dts)]
    return keep, [a.ctypes.data for a in keep]


class ForwardBackward:
    """A database of alignment pairs resident on the GPU (dnas_fb): load once, run the E-step many times."""

    def __init__(self, pairs, device=0):
        """pairs: a StockholmDB, the packed dict of its arrays(), or None (an empty handle: load() later).
        device=-1: every GPU of the node, the pairs dealt over them (counts equal one device's to 1e-12 relative)."""
        self._h = ctypes.c_void_p()
        self.n = 0
        _l.check(_l.lib().dnas_fb_create(int(device), ctypes.byref(self._h)))
        if pairs is not None:
            self.load(pairs)

    def load(self, pairs):
        """dnas_fb_load_pairs: the database goes to the GPU (replacing the one that was there)."""
        pk = pairs.arrays() if isinstance(pairs, StockholmDB) else pairs
        keep, ptrs = _pair_ptrs(pk)          # (keep: the arrays must outlive the call)
        self.n = int(pk["n"])
        _l.check(_l.lib().dnas_fb_load_pairs(self._h, self.n, *ptrs))

    def expectedCounts(self, params, strict=False, want_pair_ll=True):
        """-> (counts float64[21+P], ll, per-pair ll float64[n] or None)."""
        counts = np.zeros(21 + params.c.n_len)
        ll = ctypes.c_double()
        per = np.zeros(max(self.n, 1)) if want_pair_ll else None
        _l.check(_l.lib().dnas_fb_estep(self._h, ctypes.byref(params.c), int(bool(strict)), counts.ctypes.data, ctypes.addressof(ll),
                                        per.ctypes.data if want_pair_ll else None))
        return counts, ll.value, (per[:self.n] if want_pair_ll else None)

    @property
    def devices(self):
        """How many devices share the handle (dnas_fb_devices)."""
        return _l.lib().dnas_fb_devices(self._h)

    def stats(self):
        s = _l.FbStatsC()
        _l.check(_l.lib().dnas_fb_last_stats(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _l.lib().dnas_fb_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def expectedCounts(params, pairs, strict=False, device=0):
    """expectedCounts(params, db, ll, strict) (fwdback.cpp:190-209) on the GPU.
    pairs: StockholmDB or a dict of packed arrays (ins, in_off, outs, out_off, cm_in, cm_in_off, cm_out, cm_out_off, n).
    device=-1: every GPU of the node.  -> (counts float64[21+P], ll, per-pair ll float64[n])."""
    pk = pairs.arrays() if isinstance(pairs, StockholmDB) else pairs
    keep, ptrs = _pair_ptrs(pk)
    n = int(pk["n"])
    counts = np.zeros(21 + params.c.n_len)
    ll = ctypes.c_double()
    per = np.zeros(max(n, 1))
    _l.check(_l.lib().dnas_fwdback_estep(ctypes.byref(params.c), int(bool(strict)), n, *ptrs, int(device), counts.ctypes.data,
                                         ctypes.addressof(ll), per.ctypes.data))
    return counts, ll.value, per[:n]


def baumWelchParams(init, pairs, strict=False, device=0):
    """baumWelchParams(init, Laplace prior, db, strict) (fwdback.cpp:211-230) -> (fitted MutatorParams, iterations).
    device=-1: every GPU of the node."""
    pk = pairs.arrays() if isinstance(pairs, StockholmDB) else pairs
    keep, ptrs = _pair_ptrs(pk)
    out = _l.MutatorParamsC()
    it = ctypes.c_int32()
    _l.check(_l.lib().dnas_baum_welch(ctypes.byref(init.c), int(bool(strict)), int(pk["n"]), *ptrs, int(device), ctypes.byref(out),
                                      ctypes.addressof(it)))
    return MutatorParams(out), it.value


def mutatorScores(params):
    """dnas_mutator_scores: float64[21 + P] = delOpen, tanDup, noGap, delExtend, delEnd, sub[16], len[] -- the logarithms as the
    kernels receive them."""
    out = np.zeros(21 + params.c.n_len)
    _l.check(_l.lib().dnas_mutator_scores(ctypes.byref(params.c), out.ctypes.data))
    return out


def _tokens(seq):
    if isinstance(seq, (str, bytes)):
        return tokenize(seq).astype(np.int8)
    return np.ascontiguousarray(seq, dtype=np.int8)


def _concat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        off[1:] = np.cumsum([len(t) for t in seqs])
    data = np.concatenate(seqs).astype(np.int8) if seqs and off[-1] else np.zeros(1, np.int8)
    return np.ascontiguousarray(data), off


class PairAlignments:
    """What alignPairs returns: per pair .score float64[n], .status uint8[n] (dnas.lib.ALIGN_*), .ops (list of uint8 arrays,
    one byte per alignment column: kind | n << 2); .skipped: the indices of the pairs packed() and stockholm() leave out (no
    path, too large for the arena, or an alignment without a column); .stats: dnas_align_stats of the call (None with host=True)."""

    def __init__(self, params, ins, outs, score, status, ops, stats):
        self.params, self.ins, self.outs = params, ins, outs
        self.score, self.status, self.ops, self.stats = score, status, ops, stats
        self.skipped = [i for i in range(len(ops)) if status[i] != _l.ALIGN_OK or len(ops[i]) == 0]

    def __len__(self):
        return len(self.ops)

    def _expand(self, i, want_counts):
        a, b, ops = self.ins[i], self.outs[i], np.ascontiguousarray(self.ops[i], dtype=np.uint8)
        if self.status[i] != _l.ALIGN_OK:
            raise ValueError("pair %d has no alignment (status %d)" % (i, self.status[i]))
        n_len = self.params.c.n_len
        r1, r2 = ctypes.create_string_buffer(len(ops) + 1), ctypes.create_string_buffer(len(ops) + 1)
        cm_in, cm_out = np.zeros(len(a) + 1, np.int32), np.zeros(len(b) + 1, np.int32)
        counts = np.zeros(21 + n_len)
        ptr = lambda x: x.ctypes.data if len(x) else None
        _l.check(_l.lib().dnas_alignment_expand(n_len, ptr(a), len(a), ptr(b), len(b), ptr(ops), len(ops), r1, r2, cm_in.ctypes.data,
                                                cm_out.ctypes.data, counts.ctypes.data if want_counts else None))
        return r1.value.decode(), r2.value.decode(), cm_in, cm_out, counts

    def rows(self, i):
        """The two gapped rows of pair i (upper case, '-')."""
        return self._expand(i, False)[:2]

    def counts(self, i):
        """The moves of pair i's path in MutatorCounts order, float64[21 + P]."""
        return self._expand(i, True)[4]

    def kept(self):
        skip = set(self.skipped)
        return [i for i in range(len(self.ops)) if i not in skip]

    def packed(self):
        """The aligned pairs as the dict ForwardBackward / baumWelchParams / expectedCounts take."""
        keep = self.kept()
        parts = [self._expand(i, False) for i in keep]
        ins, in_off = _concat([self.ins[i] for i in keep])
        outs, out_off = _concat([self.outs[i] for i in keep])
        cat = lambda xs: np.concatenate(xs).astype(np.int32) if xs else np.zeros(0, np.int32)
        cm_in, cm_out = cat([p[2] for p in parts]), cat([p[3] for p in parts])
        offs = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
        return dict(ins=ins[:in_off[-1]], in_off=in_off, outs=outs[:out_off[-1]], out_off=out_off, cm_in=cm_in,
                    cm_in_off=offs([p[2] for p in parts]), cm_out=cm_out, cm_out_off=offs([p[3] for p in parts]), n=len(keep))

    def stockholm(self, names_in=None, names_out=None):
        """dnas_stockholm_write over the aligned pairs -> the text of a database --fit-error and --error-counts read.  Names
        default to in<i> / out<i>; one name in names_in serves every pair."""
        keep = self.kept()
        n = len(self.ops)
        if names_in is not None and len(names_in) == 1 and n != 1:
            names_in = list(names_in) * n
        ni = [(names_in[i] if names_in is not None else "in%d" % i).encode() for i in keep]
        no = [(names_out[i] if names_out is not None else "out%d" % i).encode() for i in keep]
        rows = [self._expand(i, False)[:2] for i in keep]
        arr = lambda xs: (ctypes.c_char_p * max(len(xs), 1))(*xs)
        text, size = ctypes.c_void_p(), ctypes.c_size_t()
        _l.check(_l.lib().dnas_stockholm_write(len(keep), arr(ni), arr(no), arr([r[0].encode() for r in rows]),
                                               arr([r[1].encode() for r in rows]), ctypes.byref(text), ctypes.byref(size)))
        out = ctypes.string_at(text, size.value).decode()
        _l.lib().dnas_free(text)
        return out


def alignPairs(params, originals, reads, band=32, device=0, arena_bytes=0, host=False):
    """dnas_align_pairs: the most probable path of the mutator pair HMM between each original and its read, on the GPU
    (host=True: dnas_align_pairs_host, no GPU).  originals, reads: lists of str or of base-code arrays; one original pairs with
    every read.  band=-1: the full matrix; device=-1: every GPU of the node.  -> PairAlignments."""
    reads = [_tokens(r) for r in reads]
    originals = [_tokens(o) for o in originals]
    if len(originals) == 1 and len(reads) != 1:
        originals = originals * len(reads)
    if len(originals) != len(reads):
        raise ValueError("%d originals for %d reads" % (len(originals), len(reads)))
    n = len(reads)
    ins, in_off = _concat(originals)
    outs, out_off = _concat(reads)
    ops_off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        ops_off[1:] = np.cumsum([len(a) + len(b) for a, b in zip(originals, reads)])
    ops = np.zeros(max(int(ops_off[-1]), 1), dtype=np.uint8)
    n_ops = np.zeros(max(n, 1), dtype=np.uint32)
    score = np.zeros(max(n, 1))
    status = np.zeros(max(n, 1), dtype=np.uint8)
    stats = None
    if host:
        _l.check(_l.lib().dnas_align_pairs_host(ctypes.byref(params.c), int(band), n, ins.ctypes.data, in_off.ctypes.data,
                                                outs.ctypes.data, out_off.ctypes.data, ops.ctypes.data, ops_off.ctypes.data,
                                                n_ops.ctypes.data, score.ctypes.data, status.ctypes.data))
    else:
        st = _l.AlignStatsC()
        _l.check(_l.lib().dnas_align_pairs(ctypes.byref(params.c), int(band), n, ins.ctypes.data, in_off.ctypes.data,
                                           outs.ctypes.data, out_off.ctypes.data, int(device), int(arena_bytes), ops.ctypes.data,
                                           ops_off.ctypes.data, n_ops.ctypes.data, score.ctypes.data, status.ctypes.data,
                                           ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    per = [ops[int(ops_off[i]):int(ops_off[i]) + int(n_ops[i])].copy() for i in range(n)]
    return PairAlignments(params, originals, reads, score[:n], status[:n], per, stats)


def pairLikelihoods(params, originals, reads, band=32, read_strand=None, device=0, host=False, exact=False):
    """dnas_pair_likelihoods: log P(read | original) under the mutator pair HMM, summed over every alignment inside the band, on
    the GPU (host=True: dnas_pair_likelihoods_host, no GPU).  originals, reads: lists of str or of base-code arrays; one original
    pairs with every read, as in alignPairs.  read_strand: None, or 0 / 1 per read (1: the read is scored as its reverse
    complement); band=-1: the full matrix; device=-1: every GPU of the node.  exact=True (host only): the log-sum-exp of the host
    libm in place of the reference's table.  -> float64[n], -inf where the band holds no path."""
    if exact and not host:
        raise ValueError("exact=True is a mode of the host statement: pass host=True")
    reads = [_tokens(r) for r in reads]
    originals = [_tokens(o) for o in originals]
    if len(originals) == 1 and len(reads) != 1:
        originals = originals * len(reads)
    if len(originals) != len(reads):
        raise ValueError("%d originals for %d reads" % (len(originals), len(reads)))
    n = len(reads)
    if read_strand is not None and len(read_strand) != n:
        raise ValueError("read_strand must hold one value per read")
    ins, in_off = _concat(originals)
    outs, out_off = _concat(reads)
    rev = None if read_strand is None else np.array([1 if x else 0 for x in read_strand] + [0], dtype=np.uint8)
    ll = np.zeros(max(n, 1))
    head = [ctypes.byref(params.c), int(band), n, ins.ctypes.data, in_off.ctypes.data, outs.ctypes.data, out_off.ctypes.data,
            None if rev is None else rev.ctypes.data]
    if host:
        _l.check(_l.lib().dnas_pair_likelihoods_host(*head, 1 if exact else 0, ll.ctypes.data))
    else:
        st = _l.ForwardStatsC()
        _l.check(_l.lib().dnas_pair_likelihoods(*head, int(device), ll.ctypes.data, ctypes.byref(st)))
        pairLikelihoods.last_stats = {k: getattr(st, k) for k, _ in st._fields_}
    return ll[:n]


pairLikelihoods.last_stats = None      # dnas_forward_stats of the last GPU call


class PairCounts:
    """What pairCounts returns: .counts float64[21 + P] and .ll, the sums over the OK pairs in pair order; per pair .pair_counts
    float64[n, 21 + P], .pair_ll (the forward score Z), .pair_ll_backward (B_S(0,0)), .status uint8[n] (lib.COUNTS_*); .stats:
    dnas_counts_stats of a GPU call as a dict, None on the host."""

    def __init__(self, counts, ll, pair_counts, pair_ll, pair_ll_backward, status, stats):
        self.counts, self.ll, self.pair_counts, self.pair_ll = counts, ll, pair_counts, pair_ll
        self.pair_ll_backward, self.status, self.stats = pair_ll_backward, status, stats


def _pair_lists(originals, reads, read_strand):
    reads = [_tokens(r) for r in reads]
    originals = [_tokens(o) for o in originals]
    if len(originals) == 1 and len(reads) != 1:
        originals = originals * len(reads)
    if len(originals) != len(reads):
        raise ValueError("%d originals for %d reads" % (len(originals), len(reads)))
    n = len(reads)
    if read_strand is not None and len(read_strand) != n:
        raise ValueError("read_strand must hold one value per read")
    ins, in_off = _concat(originals)
    outs, out_off = _concat(reads)
    rev = None if read_strand is None else np.array([1 if x else 0 for x in read_strand] + [0], dtype=np.uint8)
    keep = (ins, in_off, outs, out_off, rev)
    return n, keep, [ins.ctypes.data, in_off.ctypes.data, outs.ctypes.data, out_off.ctypes.data, None if rev is None else rev.ctypes.data]


def pairCounts(params, originals, reads, band=32, read_strand=None, device=0, arena_bytes=0, host=False, exact=False):
    """dnas_pair_counts: the posterior expected count of every move of the mutator pair HMM over every alignment inside the
    band, per pair and summed -- the E-step without a guide alignment -- on the GPU (host=True: dnas_pair_counts_host, no GPU).
    originals, reads, band, read_strand, device, exact: as pairLikelihoods.  arena_bytes: what the parked forward cells of all
    waves may take (0: what the call needs, up to half of the free HBM); a pair that alone needs more has status
    lib.COUNTS_TOO_LARGE.  -> PairCounts."""
    if exact and not host:
        raise ValueError("exact=True is a mode of the host statement: pass host=True")
    n, keep, ptrs = _pair_lists(originals, reads, read_strand)
    nc = 21 + params.c.n_len
    counts, ll = np.zeros(nc), ctypes.c_double()
    per = np.zeros((max(n, 1), nc))
    pll, back, status = np.zeros(max(n, 1)), np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.uint8)
    outs = [counts.ctypes.data, ctypes.addressof(ll), per.ctypes.data, pll.ctypes.data, back.ctypes.data, status.ctypes.data]
    stats = None
    if host:
        _l.check(_l.lib().dnas_pair_counts_host(ctypes.byref(params.c), int(band), n, *ptrs, 1 if exact else 0, *outs))
    else:
        st = _l.CountsStatsC()
        _l.check(_l.lib().dnas_pair_counts(ctypes.byref(params.c), int(band), n, *ptrs, int(device), int(arena_bytes), *outs,
                                           ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    return PairCounts(counts, ll.value, per[:n], pll[:n], back[:n], status[:n], stats)


class PairProfiles:
    """What pairProfiles returns.  .profile float64[5 + P, n_pos] (planes lib.PROFILE_SAME, _TRANSITION, _TRANSVERSION,
    _SUM_DEL_OPEN, _SUM_DEL_EXTEND, _SUM_DUP + k) and .coverage int64[n_pos]: the expected counts per position summed over the OK
    pairs in pair order, and the number of OK pairs with a row there; n_pos = max(I) + 1, position p counted from .anchor ("start":
    the 5' end, "end": the 3' end).  .pair_profiles: None, or per pair a float64[6 + P, I + 1] array (planes lib.PROFILE_MATCH + y,
    _DEL_OPEN, _DEL_EXTEND, _DUP + k; zeros for a pair that is not OK).  .pair_ll (Z), .status uint8[n] (lib.COUNTS_*); .stats:
    dnas_counts_stats of a GPU call as a dict, None on the host."""

    def __init__(self, anchor, profile, coverage, pair_profiles, pair_ll, status, stats):
        self.anchor, self.profile, self.coverage, self.pair_profiles = anchor, profile, coverage, pair_profiles
        self.pair_ll, self.status, self.stats = pair_ll, status, stats

    def rates(self):
        """-> dict of float64[n_pos]: 'substitution' (transitions + transversions), 'deletion' (opened + extended) and
        'duplication' (every length) per position, each the expected count over the coverage (NaN where nothing covers)."""
        p = self.profile
        with np.errstate(invalid="ignore", divide="ignore"):
            cov = self.coverage.astype(np.float64)
            return {"substitution": (p[_l.PROFILE_TRANSITION] + p[_l.PROFILE_TRANSVERSION]) / cov,
                    "deletion": (p[_l.PROFILE_SUM_DEL_OPEN] + p[_l.PROFILE_SUM_DEL_EXTEND]) / cov,
                    "duplication": p[_l.PROFILE_SUM_DUP:].sum(axis=0) / cov}


def pairProfiles(params, originals, reads, band=32, read_strand=None, device=0, arena_bytes=0, host=False, exact=False,
                 anchor="start", per_pair=True):
    """dnas_pair_profiles: the posteriors of pairCounts kept per base of the original -- where along each strand the
    substitutions, deletions and duplications probably fell -- per pair and summed per position, on the GPU (host=True:
    dnas_pair_profiles_host, no GPU).  originals, reads, band, read_strand, device, arena_bytes, exact: as pairCounts.  anchor:
    "start" or "end", the end of the original the aggregate's positions count from; per_pair=False: the aggregate only.
    -> PairProfiles."""
    if exact and not host:
        raise ValueError("exact=True is a mode of the host statement: pass host=True")
    if anchor not in ("start", "end"):
        raise ValueError("anchor must be 'start' or 'end'")
    n, keep, ptrs = _pair_lists(originals, reads, read_strand)
    in_off = keep[1]
    W, n_pos = 6 + params.c.n_len, (int(np.diff(in_off).max()) + 1 if n else 0)
    profile, coverage = np.zeros((W - 1, max(n_pos, 1))), np.zeros(max(n_pos, 1), dtype=np.int64)
    blocks = np.zeros(max(W * (int(in_off[-1]) + n), 1)) if per_pair else None
    pll, status = np.zeros(max(n, 1)), np.zeros(max(n, 1), dtype=np.uint8)
    tail = [_l.PROFILE_FROM_END if anchor == "end" else _l.PROFILE_FROM_START, n_pos, profile.ctypes.data, coverage.ctypes.data,
            None if blocks is None else blocks.ctypes.data, pll.ctypes.data, status.ctypes.data]
    stats = None
    if host:
        _l.check(_l.lib().dnas_pair_profiles_host(ctypes.byref(params.c), int(band), n, *ptrs, 1 if exact else 0, *tail))
    else:
        st = _l.CountsStatsC()
        _l.check(_l.lib().dnas_pair_profiles(ctypes.byref(params.c), int(band), n, *ptrs, int(device), int(arena_bytes), *tail,
                                             ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    per = None
    if per_pair:
        per = [blocks[W * (int(in_off[i]) + i):W * (int(in_off[i + 1]) + i + 1)].reshape(W, -1) for i in range(n)]
    return PairProfiles(anchor, profile[:, :n_pos], coverage[:n_pos], per, pll[:n], status[:n], stats)


def baumWelchPairs(init, originals, reads, band=32, read_strand=None, device=0, max_iterations=0, host=False, exact=False,
                   arena_bytes=0):
    """dnas_baum_welch_pairs: the EM of baumWelchParams over pairCounts -- the error model fitted from unaligned (original,
    read) pairs, every alignment inside the band summed at every iteration (host=True: dnas_baum_welch_pairs_host).
    max_iterations=0: 100.  -> (fitted MutatorParams, iterations, trace); trace: one (MutatorParams, ll + log prior) per E-step
    that was run, the one that stopped the loop included."""
    if exact and not host:
        raise ValueError("exact=True is a mode of the host statement: pass host=True")
    n, keep, ptrs = _pair_lists(originals, reads, read_strand)
    room = int(max_iterations) if max_iterations else 100
    out, it, n_trace = _l.MutatorParamsC(), ctypes.c_int32(), ctypes.c_int32()
    tp = (_l.MutatorParamsC * max(room, 1))()
    tll = np.zeros(max(room, 1))
    tail = [int(max_iterations), ctypes.byref(out), ctypes.addressof(it), ctypes.addressof(tp), tll.ctypes.data,
            ctypes.addressof(n_trace)]
    if host:
        _l.check(_l.lib().dnas_baum_welch_pairs_host(ctypes.byref(init.c), int(band), n, *ptrs, 1 if exact else 0, *tail))
    else:
        _l.check(_l.lib().dnas_baum_welch_pairs(ctypes.byref(init.c), int(band), n, *ptrs, int(device), int(arena_bytes), *tail))
    trace = []
    for i in range(n_trace.value):
        c = _l.MutatorParamsC()
        ctypes.memmove(ctypes.addressof(c), ctypes.addressof(tp[i]), ctypes.sizeof(c))
        trace.append((MutatorParams(c), float(tll[i])))
    return MutatorParams(out), it.value, trace


class ReadAssignments:
    """What assignReads returns, per read: .original int64[N] (-1: none), .strand uint8[N] (1: the read's reverse complement
    matched), .score and .second float64[N] (the best item's score, and the best among the items of another original),
    .margin = score - second (inf with a single original, -inf for an unassigned read), .status uint8[N] (dnas.lib.ASSIGN_*);
    .stats: dnas_assign_stats of the call (None with host=True); .item_scores: None, or per read the float64 array of its
    items' scores in item order."""

    def __init__(self, originals, reads, original, strand, score, second, status, stats, item_scores):
        self.originals, self.reads = originals, reads
        self.original, self.strand, self.score, self.second, self.status = original, strand, score, second, status
        self.stats, self.item_scores = stats, item_scores
        with np.errstate(invalid="ignore"):
            self.margin = np.where(original >= 0, score - second, -np.inf)

    def __len__(self):
        return len(self.original)

    def pairs(self, min_margin=0.):
        """-> (originals_for_reads, oriented_reads, kept_indices): the reads assigned with a margin of at least min_margin, each
        reverse-complemented where its strand says so, beside its original -- what alignPairs takes."""
        kept = [i for i in range(len(self)) if self.original[i] >= 0 and self.margin[i] >= min_margin]
        ins = [self.originals[int(self.original[i])] for i in kept]
        outs = [reverse_complement(self.reads[i]).astype(np.int8) if self.strand[i] else self.reads[i] for i in kept]
        return ins, outs, kept


def _candidates(candidates, n):
    """None, or one list of original indices per read -> (cand_off, cand_idx) of the CSR form."""
    if candidates is None:
        return None, None
    if len(candidates) != n:
        raise ValueError("%d candidate lists for %d reads" % (len(candidates), n))
    off = np.zeros(n + 1, dtype=np.int64)
    if n:
        off[1:] = np.cumsum([len(c) for c in candidates])
    idx = np.array([int(x) for c in candidates for x in c] + [0], dtype=np.int64)
    return off, idx


class Assigner:
    """dnas_assigner: the originals of a library kept on the GPU (device=-1: on every GPU of the node); .assign(reads, ...)
    assigns one pool after another to them."""

    def __init__(self, params, originals, band=32, device=0):
        self.params = params
        self.originals = [_tokens(o) for o in originals]
        seqs, off = _concat(self.originals)
        self.h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_assigner_create(ctypes.byref(params.c), int(band), len(self.originals), seqs.ctypes.data,
                                               off.ctypes.data, int(device), ctypes.byref(self.h)))

    def assign(self, reads, strands="both", candidates=None, item_scores=False):
        return _assign(self, self.params, self.originals, reads, 0, strands, candidates, 0, False, item_scores)

    def close(self):
        if getattr(self, "h", None):
            _l.lib().dnas_assigner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _assign(handle, params, originals, reads, band, strands, candidates, device, host, item_scores):
    reads = [_tokens(r) for r in reads]
    n, K = len(reads), len(originals)
    mode = _l.strand_mode(strands)
    outs, out_off = _concat(reads)
    cand_off, cand_idx = _candidates(candidates, n)
    per_read = np.diff(cand_off) if cand_off is not None else np.full(n, K, dtype=np.int64)
    item_off = np.concatenate([[0], np.cumsum(per_read)]).astype(np.int64) * (2 if mode == _l.STRAND_BOTH else 1)
    original = np.zeros(max(n, 1), dtype=np.int64)
    strand, status = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    score, second = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    items = np.zeros(int(item_off[-1]) + 1) if item_scores else None
    ptr = lambda x: x.ctypes.data if x is not None else None
    tail = [ptr(original), ptr(strand), ptr(score), ptr(second), ptr(status), ptr(items)]
    stats = None
    if handle is not None:
        st = _l.AssignStatsC()
        _l.check(_l.lib().dnas_assigner_run(handle.h, n, ptr(outs), ptr(out_off), mode, ptr(cand_off), ptr(cand_idx), *tail,
                                            ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    else:
        ins, in_off = _concat(originals)
        head = [ctypes.byref(params.c), int(band), K, ptr(ins), ptr(in_off), n, ptr(outs), ptr(out_off), mode, ptr(cand_off),
                ptr(cand_idx)]
        if host:
            _l.check(_l.lib().dnas_assign_reads_host(*head, *tail))
        else:
            st = _l.AssignStatsC()
            _l.check(_l.lib().dnas_assign_reads(*head, int(device), *tail, ctypes.byref(st)))
            stats = {k: getattr(st, k) for k, _ in st._fields_}
    per = [items[int(item_off[i]):int(item_off[i + 1])].copy() for i in range(n)] if item_scores else None
    return ReadAssignments(originals, reads, original[:n], strand[:n], score[:n], second[:n], status[:n], stats, per)


def assignReads(params, originals, reads, band=32, strands="both", candidates=None, device=0, host=False, item_scores=False):
    """dnas_assign_reads: per read of a shuffled pool, the original and the orientation under which the pair-HMM score of
    alignPairs is largest, on the GPU (host=True: dnas_assign_reads_host, no GPU).  originals, reads: lists of str or of
    base-code arrays; strands: 'forward', 'reverse' or 'both'; candidates: None (every original) or, per read, the list of
    original indices to try, in that order; band=-1: the full matrix; device=-1: every GPU of the node.  -> ReadAssignments."""
    return _assign(None, params, [_tokens(o) for o in originals], reads, band, strands, candidates, device, host, item_scores)


class ClusterConsensus:
    """What consensusScore returns, per cluster: .winner int64[C] (an index into the cluster's own candidate list, -1: none),
    .total and .second float64[C] (the winner's joint score, and the best among the cluster's other candidates), .margin =
    total - second (inf with a single candidate, -inf without a winner), .status uint8[C] (dnas.lib.CONSENSUS_*); .totals: per
    cluster the float64 array of its candidates' totals; .stats: dnas_consensus_stats of the call (None with host=True).  With
    score="forward" also .posterior (per cluster the float64 array of P(candidate | reads), uniform prior over the listed
    candidates; zeros unless the status is CONSENSUS_OK) and .confidence float64[C] (the winner's posterior, 0 without a winner)."""

    def __init__(self, winner, total, second, status, totals, stats, posterior=None):
        self.winner, self.total, self.second, self.status, self.totals, self.stats = winner, total, second, status, totals, stats
        if posterior is not None:
            self.posterior = posterior
            self.confidence = np.array([p[int(w)] if w >= 0 else 0. for p, w in zip(posterior, winner)], dtype=np.float64)
        with np.errstate(invalid="ignore"):
            self.margin = np.where(winner >= 0, total - second, -np.inf)

    def __len__(self):
        return len(self.winner)


class ClusterDecodes:
    """What ViterbiDecoder.decode_clusters returns, per cluster in order of first appearance: .labels, .symbols (the winning
    message, '' without a winner), .read (the index, in the caller's read list, of the first read that decoded to the winner's
    strand; -1), .total, .second, .margin, .votes (reads whose messages encode to the winner's strand), .n_candidates, .status
    (dnas.lib.CONSENSUS_*); .per_read: what decode(reads, strands) returns with a strand array, in the caller's read order;
    .stats: dnas_consensus_stats of the call.  .source uint8[C]: 1 where the message is the consensus read's (polish > 0; .read
    is -1 there), else 0; .consensus_reads: None without polishing, else the consensus reads as strings; .consensus_decodes:
    None, or (symbols, loglike, status) of their decode.  With score="forward" also .confidence float64[C]: the winner's posterior
    among the cluster's candidates (0 without a winner); the default call has no such attribute."""

    def __init__(self, labels, symbols, read, total, second, votes, n_candidates, status, per_read, stats):
        self.labels, self.symbols, self.read, self.total, self.second = labels, symbols, read, total, second
        self.votes, self.n_candidates, self.status, self.per_read, self.stats = votes, n_candidates, status, per_read, stats
        self.source, self.consensus_reads, self.consensus_decodes = np.zeros(len(labels), dtype=np.uint8), None, None
        with np.errstate(invalid="ignore"):
            self.margin = np.where(read >= 0, total - second, -np.inf)

    def __len__(self):
        return len(self.labels)


def consensusScore(params, candidates, reads, band=32, read_strand=None, device=0, host=False, score="viterbi"):
    """dnas_consensus_score: per cluster, the candidate strand under which the cluster's reads have the largest summed pair-HMM
    score of alignPairs, on the GPU (host=True: dnas_consensus_score_host, no GPU).  candidates, reads: one list per cluster of
    str or base-code arrays; read_strand: None, or per cluster a list of 0 / 1 per read (1: the read is scored as its reverse
    complement); band=-1: the full matrix; device=-1: every GPU of the node.  score="forward" (dnas_consensus_score_ex): an item's
    score is the marginal likelihood of pairLikelihoods instead of the best alignment's score, and the result carries .posterior
    and .confidence.  -> ClusterConsensus."""
    smode = _l.score_mode(score)
    if len(candidates) != len(reads):
        raise ValueError("%d candidate lists for %d clusters of reads" % (len(candidates), len(reads)))
    if read_strand is not None and [len(x) for x in read_strand] != [len(x) for x in reads]:
        raise ValueError("read_strand must hold one value per read")
    nc = len(reads)
    cand = [_tokens(x) for c in candidates for x in c]
    rds = [_tokens(x) for c in reads for x in c]
    offs = lambda groups: np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    cl_cand, cl_read = offs(candidates), offs(reads)
    cseq, coff = _concat(cand)
    rseq, roff = _concat(rds)
    strand = None if read_strand is None else np.array([int(x) for c in read_strand for x in c] + [0], dtype=np.uint8)
    winner = np.zeros(max(nc, 1), dtype=np.int64)
    total, second = np.zeros(max(nc, 1)), np.zeros(max(nc, 1))
    status = np.zeros(max(nc, 1), dtype=np.uint8)
    totals = np.zeros(len(cand) + 1)
    ptr = lambda x: x.ctypes.data if x is not None else None
    head = [ctypes.byref(params.c), int(band), nc, len(cand), ptr(cseq), ptr(coff), ptr(cl_cand), len(rds), ptr(rseq), ptr(roff),
            ptr(strand), ptr(cl_read)]
    tail = [ptr(winner), ptr(total), ptr(second), ptr(status), ptr(totals)]
    stats = None
    post = np.zeros(len(cand) + 1) if smode != _l.SCORE_VITERBI else None
    if smode != _l.SCORE_VITERBI:
        if host:
            _l.check(_l.lib().dnas_consensus_score_host_ex(*head, smode, *tail, ptr(post)))
        else:
            st = _l.ConsensusStatsC()
            _l.check(_l.lib().dnas_consensus_score_ex(*head, int(device), smode, *tail, ptr(post), ctypes.byref(st)))
            stats = {k: getattr(st, k) for k, _ in st._fields_}
    elif host:
        _l.check(_l.lib().dnas_consensus_score_host(*head, *tail))
    else:
        st = _l.ConsensusStatsC()
        _l.check(_l.lib().dnas_consensus_score(*head, int(device), *tail, ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    local = np.where(winner[:nc] >= 0, winner[:nc] - cl_cand[:nc], -1)
    per = [totals[int(cl_cand[c]):int(cl_cand[c + 1])].copy() for c in range(nc)]
    per_post = None if post is None else [post[int(cl_cand[c]):int(cl_cand[c + 1])].copy() for c in range(nc)]
    return ClusterConsensus(local, total[:nc], second[:nc], status[:nc], per, stats, per_post)


class ConsensusReads:
    """What consensusReads returns, per cluster: .seqs (the consensus reads, int8 base-code arrays), .rounds int32[C] (rounds that
    changed the template), .converged uint8[C] (1: a round returned the template it was given), .voters int32[C] and .status
    uint8[C] (dnas.lib.POLISH_*) of the last round that ran; .stats: dnas_polish_stats of the call (None with host=True)."""

    def __init__(self, seqs, rounds, converged, voters, status, stats):
        self.seqs, self.rounds, self.converged, self.voters, self.status, self.stats = seqs, rounds, converged, voters, status, stats

    def __len__(self):
        return len(self.seqs)

    def strings(self):
        return ["".join("ACGT"[b] for b in s) for s in self.seqs]


def consensusReads(params, templates, reads, band=32, read_strand=None, rounds=4, device=0, arena_bytes=0, host=False):
    """dnas_cluster_consensus: per cluster, the reads aligned to the template under the pair HMM of alignPairs and column-voted
    into a new template, for at most `rounds` rounds or until a round changes nothing, on the GPU (host=True:
    dnas_cluster_consensus_host, no GPU).  templates: one str or base-code array per cluster; reads: one list per cluster;
    read_strand: None, or per cluster a list of 0 / 1 per read (1: the read votes as its reverse complement); band=-1: the full
    matrix; device=-1: every GPU of the node.  -> ConsensusReads."""
    if len(templates) != len(reads):
        raise ValueError("%d templates for %d clusters of reads" % (len(templates), len(reads)))
    if read_strand is not None and [len(x) for x in read_strand] != [len(x) for x in reads]:
        raise ValueError("read_strand must hold one value per read")
    nc = len(reads)
    tmpl = [_tokens(t) for t in templates]
    rds = [_tokens(x) for c in reads for x in c]
    cl_read = np.concatenate([[0], np.cumsum([len(g) for g in reads])]).astype(np.int64)
    tseq, toff = _concat(tmpl)
    rseq, roff = _concat(rds)
    strand = None if read_strand is None else np.array([int(x) for c in read_strand for x in c] + [0], dtype=np.uint8)
    out_seqs, out_off = ctypes.c_void_p(), np.zeros(nc + 1, dtype=np.int64)
    n_rounds, voters = np.zeros(max(nc, 1), dtype=np.int32), np.zeros(max(nc, 1), dtype=np.int32)
    converged, status = np.zeros(max(nc, 1), dtype=np.uint8), np.zeros(max(nc, 1), dtype=np.uint8)
    ptr = lambda x: x.ctypes.data if x is not None else None
    head = [ctypes.byref(params.c), int(band), nc, ptr(tseq), ptr(toff), len(rds), ptr(rseq), ptr(roff), ptr(strand), ptr(cl_read),
            int(rounds)]
    tail = [ctypes.byref(out_seqs), ptr(out_off), ptr(n_rounds), ptr(converged), ptr(voters), ptr(status)]
    stats = None
    if host:
        _l.check(_l.lib().dnas_cluster_consensus_host(*head, *tail))
    else:
        st = _l.PolishStatsC()
        _l.check(_l.lib().dnas_cluster_consensus(*head, int(device), int(arena_bytes), *tail, ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    flat = _take(out_seqs, ctypes.c_int8, int(out_off[nc]), np.int8)
    seqs = [flat[int(out_off[c]):int(out_off[c + 1])].copy() for c in range(nc)]
    return ConsensusReads(seqs, n_rounds[:nc], converged[:nc], voters[:nc], status[:nc], stats)


class ReadClusters:
    """What clusterReads returns, per read: .cluster int64[N] (dense ids in order of first appearance), .root int64[N] (the
    smallest read index of the read's cluster), .strand uint8[N] (1: reverse-complemented relative to the root), .status
    uint8[N] (dnas.lib.CLUSTER_*); .n_clusters; .sizes int64[n_clusters]; .edges: None, or (ij int64[E, 2], score float64[E],
    strand uint8[E]) sorted by (i, j); .stats: dnas_cluster_stats of the call (host=True: the counts, the times 0); .gate:
    dnas_cluster_gate_stats of a call with max_edit_permille >= 0, else None."""

    def __init__(self, cluster, root, strand, status, edges, stats, gate=None):
        self.cluster, self.root, self.strand, self.status, self.edges, self.stats = cluster, root, strand, status, edges, stats
        self.gate = gate
        self.n_clusters = int(cluster.max()) + 1 if len(cluster) else 0
        self.sizes = np.bincount(cluster, minlength=self.n_clusters).astype(np.int64)

    def __len__(self):
        return len(self.cluster)

    def labels(self):
        """One label per read, as ViterbiDecoder.decode_clusters takes them."""
        return [int(c) for c in self.cluster]


def _take(ptr, ctype, count, dtype):
    """A library-allocated array -> numpy, the library's copy freed."""
    out = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(max(count, 1),))[:count].astype(dtype, copy=True)
    _l.lib().dnas_free(ptr)
    return out


def clusterReads(params, reads, band=32, k=12, sketch=32, min_shared=2, min_score_per_nt=0.0, device=0, host=False, edges=False,
                 max_edit_permille=-1):
    """dnas_cluster_reads: the pool's reads partitioned into the connected components of the graph whose edges are the pairs
    i < j that share at least min_shared of `sketch` min-hash positions over canonical k-mers and whose pair-HMM score of read j
    as a mutated copy of read i, in the better orientation, is at least min_score_per_nt x len(read j); on the GPU (host=True:
    dnas_cluster_reads_host, no GPU).  reads: list of str or of base-code arrays; min_shared=0: no filter, every pair is scored;
    band=-1: the full matrix; device=-1: every GPU of the node; edges=True: keep the edge list; max_edit_permille >= 0: the
    edit-distance gate (dnas_cluster_reads_gated) -- only pairs whose Levenshtein distance, in the better orientation, is at most
    that many thousandths of the longer read are scored.  -> ReadClusters."""
    reads = [_tokens(r) for r in reads]
    n = len(reads)
    seqs, off = _concat(reads)
    root, cluster = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
    strand, status = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    e_ij, e_score, e_strand, n_edges = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    st = _l.ClusterStatsC()
    head = [ctypes.byref(params.c), int(band), int(k), int(sketch), int(min_shared), float(min_score_per_nt), n, seqs.ctypes.data,
            off.ctypes.data]
    ref = lambda x: ctypes.byref(x) if edges else None
    tail = [root.ctypes.data, cluster.ctypes.data, strand.ctypes.data, status.ctypes.data, ref(e_ij), ref(e_score), ref(e_strand),
            ctypes.byref(n_edges), ctypes.byref(st)]
    gs = _l.ClusterGateStatsC()
    head.insert(6, int(max_edit_permille))
    if host:
        _l.check(_l.lib().dnas_cluster_reads_gated_host(*head, *tail, ctypes.byref(gs)))
    else:
        _l.check(_l.lib().dnas_cluster_reads_gated(*head, int(device), *tail, ctypes.byref(gs)))
    gate = {k_: getattr(gs, k_) for k_, _ in gs._fields_} if int(max_edit_permille) != -1 else None
    found = None
    if edges:
        ne = n_edges.value
        found = (_take(e_ij, ctypes.c_int64, 2 * ne, np.int64).reshape(ne, 2), _take(e_score, ctypes.c_double, ne, np.float64),
                 _take(e_strand, ctypes.c_uint8, ne, np.uint8))
    return ReadClusters(cluster[:n], root[:n], strand[:n], status[:n], found, {k_: getattr(st, k_) for k_, _ in st._fields_}, gate)


class Clusterer:
    """dnas_clusterer: a pool of reads that grows by batches, kept on one GPU.  .add(reads) gives the new reads the next indices
    and examines every pair whose larger index is new, exactly as clusterReads treats a pair -> the add's own dnas_cluster_stats
    as a dict (plus "gate": the add's dnas_cluster_gate_stats with max_edit_permille >= 0, else None); .result(edges=False) -> the
    ReadClusters of the whole pool so far, equal to clusterReads on the concatenation of the batches; .n_reads; .close().  A
    context manager; a closed handle raises ValueError."""

    def __init__(self, params, band=32, k=12, sketch=32, min_shared=2, min_score_per_nt=0.0, max_edit_permille=-1, device=0):
        self.params, self.gated = params, int(max_edit_permille) != -1
        self.h = ctypes.c_void_p()
        _l.check(_l.lib().dnas_clusterer_create(ctypes.byref(params.c), int(band), int(k), int(sketch), int(min_shared),
                                                float(min_score_per_nt), int(max_edit_permille), int(device), ctypes.byref(self.h)))

    def _handle(self):
        if not getattr(self, "h", None):
            raise ValueError("the Clusterer is closed")
        return self.h

    def _gate(self, gs):
        return {k_: getattr(gs, k_) for k_, _ in gs._fields_} if self.gated else None

    @property
    def n_reads(self):
        return int(_l.lib().dnas_clusterer_reads(self._handle()))

    def add(self, reads):
        h = self._handle()
        reads = [_tokens(r) for r in reads]
        seqs, off = _concat(reads)
        st, gs = _l.ClusterStatsC(), _l.ClusterGateStatsC()
        _l.check(_l.lib().dnas_clusterer_add(h, len(reads), seqs.ctypes.data, off.ctypes.data, ctypes.byref(st), ctypes.byref(gs)))
        stats = {k_: getattr(st, k_) for k_, _ in st._fields_}
        stats["gate"] = self._gate(gs)
        return stats

    def result(self, edges=False):
        h = self._handle()
        n = self.n_reads
        root, cluster = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        strand, status = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
        e_ij, e_score, e_strand, n_edges = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
        st, gs = _l.ClusterStatsC(), _l.ClusterGateStatsC()
        ref = lambda x: ctypes.byref(x) if edges else None
        _l.check(_l.lib().dnas_clusterer_result(h, root.ctypes.data, cluster.ctypes.data, strand.ctypes.data, status.ctypes.data,
                                                ref(e_ij), ref(e_score), ref(e_strand), ctypes.byref(n_edges), ctypes.byref(st),
                                                ctypes.byref(gs)))
        found = None
        if edges:
            ne = n_edges.value
            found = (_take(e_ij, ctypes.c_int64, 2 * ne, np.int64).reshape(ne, 2), _take(e_score, ctypes.c_double, ne, np.float64),
                     _take(e_strand, ctypes.c_uint8, ne, np.uint8))
        return ReadClusters(cluster[:n], root[:n], strand[:n], status[:n], found, {k_: getattr(st, k_) for k_, _ in st._fields_},
                            self._gate(gs))

    def close(self):
        if getattr(self, "h", None):
            _l.lib().dnas_clusterer_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def editDistances(reads, pairs, device=0, host=False):
    """dnas_edit_distances: for every pair (i, j) of `pairs` (indices into reads; i = j is allowed) the Levenshtein distance of
    read i and read j, and of read i and the reverse complement of read j, exact -> int32[C, 2].  On the GPU (device=-1: every
    GPU of the node), or with host=True the two-row dynamic program on the host (dnas_edit_distances_host)."""
    reads = [_tokens(r) for r in reads]
    seqs, off = _concat(reads)
    ij = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    dist = np.zeros((max(len(ij), 1), 2), dtype=np.int32)
    if host:
        _l.check(_l.lib().dnas_edit_distances_host(len(ij), ij.ctypes.data, len(reads), seqs.ctypes.data, off.ctypes.data, dist.ctypes.data))
    else:
        _l.check(_l.lib().dnas_edit_distances(len(ij), ij.ctypes.data, len(reads), seqs.ctypes.data, off.ctypes.data, int(device),
                                              dist.ctypes.data))
    return dist[:len(ij)]


class TrimmedReads:
    """What trimReads returns, per read: .pair int32[N] (the primer pair, -1: none), .strand uint8[N] (1: the read is the reverse
    complement of the molecule), .begin and .end int32[N] (the payload in the coordinates of the read as given), .edits
    int32[N, 2] (the edits of the forward and of the reverse primer, -1: a missing anchor), .second int32[N] (the best total of
    another pair's accepted candidate, -1: none), .status uint8[N] (dnas.lib.TRIM_*); .total int64[N] (the winner's total, -1
    without one), .margin int64[N] = second - total (NO_SECOND with no second, -1 for a read without a pair); .stats:
    dnas_trim_stats of the call (None with host=True)."""

    NO_SECOND = 1 << 40

    def __init__(self, reads, as_text, pair, strand, begin, end, edits, second, status, stats, limits):
        self.reads, self.as_text, self.pair, self.strand, self.begin, self.end = reads, as_text, pair, strand, begin, end
        self.edits, self.second, self.status, self.stats = edits, second, status, stats
        # the winner's total: its edits, a missing anchor counting as its limit + 1 (limits int64[K, 2])
        won = pair >= 0
        lim = limits[np.where(won, pair, 0)] if len(limits) else np.zeros((len(pair), 2), np.int64)
        self.total = np.where(won, np.where(edits < 0, lim + 1, edits).sum(axis=1), -1).astype(np.int64)
        self.margin = np.where(won, np.where(second < 0, self.NO_SECOND, second.astype(np.int64) - self.total), -1)

    def __len__(self):
        return len(self.pair)

    def payloads(self):
        """One entry per read: the payload oriented forward -- a str where the read was given as one, else an int8 array of base
        codes; None where the status is nonzero."""
        out = []
        for i in range(len(self)):
            if self.status[i]:
                out.append(None)
                continue
            cut = self.reads[i][int(self.begin[i]):int(self.end[i])]
            cut = reverse_complement(cut).astype(np.int8) if self.strand[i] else cut
            out.append("".join("ACGT"[b] for b in cut) if self.as_text[i] else cut)
        return out

    def kept(self, pair=None, min_margin=0):
        """The indices of the trimmed reads, of primer pair `pair` only when one is named, whose margin over the best candidate of
        another pair is at least min_margin edits."""
        return [i for i in range(len(self)) if self.status[i] == 0 and (pair is None or self.pair[i] == pair)
                and self.margin[i] >= min_margin]


def trimReads(primers, reads, max_offset=8, max_edit_permille=250, anchors="both", min_payload=0, device=0, host=False):
    """dnas_trim_reads: which primer pair frames each read of a pool, on which strand, and where its payload lies.  primers: a
    list of (F, R), both as they appear on the forward strand (the molecule is F . payload . R), 1 .. 64 bases each.  A primer is
    searched within its length + max_offset columns of the read's end (-1: anywhere) and may differ by max_edit_permille
    thousandths of its length; anchors="either" accepts a read that has only one of its two primers; min_payload: the bases that
    must remain.  On the GPU (device=-1: every GPU of the node), or with host=True the dynamic program on the host
    (dnas_trim_reads_host).  -> TrimmedReads."""
    if anchors not in _l.TRIM_ANCHORS:
        raise ValueError("anchors must be 'both' or 'either', not %r" % (anchors,))
    as_text = [isinstance(r, (str, bytes)) for r in reads]
    reads = [_tokens(r) for r in reads]
    seqs, off = _concat(reads)
    flat = []
    for pr in primers:
        if len(pr) != 2:
            raise ValueError("a primer pair is (F, R)")
        flat += [_tokens(pr[0]), _tokens(pr[1])]
    pseqs, poff = _concat(flat)
    n = len(reads)
    pair, begin, end = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(3))
    second, edits = np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), 2), dtype=np.int32)
    strand, status = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint8)
    head = [len(primers), pseqs.ctypes.data, poff.ctypes.data, n, seqs.ctypes.data, off.ctypes.data, int(max_offset), int(max_edit_permille),
            _l.TRIM_ANCHORS[anchors], int(min_payload)]
    outs = [pair.ctypes.data, strand.ctypes.data, begin.ctypes.data, end.ctypes.data, edits.ctypes.data, second.ctypes.data, status.ctypes.data]
    stats = None
    if host:
        _l.check(_l.lib().dnas_trim_reads_host(*head, *outs))
    else:
        st = _l.TrimStatsC()
        _l.check(_l.lib().dnas_trim_reads(*head, int(device), *outs, ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    limits = np.array([int(max_edit_permille) * len(t) // 1000 for t in flat], dtype=np.int64).reshape(-1, 2)
    return TrimmedReads(reads, as_text, pair[:n], strand[:n], begin[:n], end[:n], edits[:n], second[:n], status[:n], stats, limits)


class SimulatedReads:
    """What simulateReads returns, per read: .reads (int8 arrays of base codes, as handed out), .strand int64[N] (the original
    it was drawn from), .reversed uint8[N] (1: handed out reverse-complemented), .ops (uint8 arrays, one byte per alignment column
    of (original, read before reversal), kind | n << 2 as alignPairs returns them; None with ops=False), .status uint8[N]
    (dnas.lib.SIM_*); .stats: dnas_simulate_stats of the call (None with host=True)."""

    def __init__(self, params, originals, reads, strand, reversed_, ops, status, stats):
        self.params, self.originals, self.reads, self.strand, self.reversed = params, originals, reads, strand, reversed_
        self.ops, self.status, self.stats = ops, status, stats

    def __len__(self):
        return len(self.reads)

    def strings(self):
        return ["".join("ACGT"[b] for b in r) for r in self.reads]

    def forward(self, i):
        """Read i before the reversal: what its ops describe."""
        return reverse_complement(self.reads[i]).astype(np.int8) if self.reversed[i] else self.reads[i]

    def _paths(self):
        if self.ops is None:
            raise ValueError("simulateReads was called with ops=False")
        return PairAlignments(self.params, [self.originals[int(s)] for s in self.strand], [self.forward(i) for i in range(len(self))],
                              np.zeros(len(self)), self.status, self.ops, None)

    def alignment(self, i):
        """dnas_alignment_expand over read i's true path: (row of the original, row of the read, counts float64[21 + P])."""
        if self.ops is None:
            raise ValueError("simulateReads was called with ops=False")
        one = PairAlignments(self.params, [self.originals[int(self.strand[i])]], [self.forward(i)], np.zeros(1), self.status[i:i + 1],
                             [self.ops[i]], None)
        r1, r2, _, _, counts = one._expand(0, True)
        return r1, r2, counts

    def stockholm(self, names_in=None, names_out=None):
        """dnas_stockholm_write over the true paths (reads without a column left out): the database --fit-error reads."""
        if names_in is None:
            names_in = ["strand%d" % int(s) for s in self.strand]
        if names_out is None:
            count, names_out = {}, []
            for s in self.strand:
                count[int(s)] = count.get(int(s), 0) + 1
                names_out.append("strand%d/%d" % (int(s), count[int(s)]))
        return self._paths().stockholm(names_in, names_out)


def simulateReads(params, originals, coverage=1, read_strand=None, seed=0, first_index=0, reverse_prob=0., shuffle=False, ops=True,
                  device=0, arena_bytes=0, host=False):
    """dnas_simulate_reads: reads of the originals sampled from the pair HMM of params, each with the path that made it, on the GPU
    (host=True: dnas_simulate_reads_host, no GPU; the two are bit-identical).  originals: a list of str or of base-code arrays.
    read_strand: the original of every read; None: coverage reads of each original, strand-major.  shuffle: read_strand is permuted
    with random.Random(seed) first.  Read i of the call is read first_index + i of the seed: a list may be drawn in pieces.
    reverse_prob: the probability that a read is handed out as its reverse complement.  device=-1: every GPU of the node.
    -> SimulatedReads."""
    originals = [_tokens(o) for o in originals]
    if read_strand is None:
        read_strand = [s for s in range(len(originals)) for _ in range(int(coverage))]
    read_strand = [int(s) for s in read_strand]
    if shuffle:
        import random
        random.Random(seed).shuffle(read_strand)
    strand = np.array(read_strand + [0], dtype=np.int64)
    n = len(read_strand)
    seqs, off = _concat(originals)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    o_seqs, o_off, o_rev, o_ops, o_ops_off = (ctypes.c_void_p() for _ in range(5))
    head = [ctypes.byref(params.c), len(originals), seqs.ctypes.data, off.ctypes.data, n, strand.ctypes.data, int(seed), int(first_index),
            float(reverse_prob), int(bool(ops))]
    outs = [ctypes.byref(o_seqs), ctypes.byref(o_off), ctypes.byref(o_rev), ctypes.byref(o_ops), ctypes.byref(o_ops_off), status.ctypes.data]
    stats = None
    if host:
        _l.check(_l.lib().dnas_simulate_reads_host(*head, *outs))
    else:
        st = _l.SimulateStatsC()
        _l.check(_l.lib().dnas_simulate_reads(*head, int(device), int(arena_bytes), *outs, ctypes.byref(st)))
        stats = {k: getattr(st, k) for k, _ in st._fields_}
    r_off = _take(o_off, ctypes.c_int64, n + 1, np.int64)
    flat = _take(o_seqs, ctypes.c_int8, int(r_off[n]), np.int8)
    rev = _take(o_rev, ctypes.c_uint8, n, np.uint8)
    reads = np.split(flat, r_off[1:n]) if n else []
    per_ops = None
    if ops:
        p_off = _take(o_ops_off, ctypes.c_int64, n + 1, np.int64)
        flat_ops = _take(o_ops, ctypes.c_uint8, int(p_off[n]), np.uint8)
        per_ops = np.split(flat_ops, p_off[1:n]) if n else []
    return SimulatedReads(params, originals, reads, strand[:n], rev, per_ops, status[:n], stats)


def framePrimers(originals, primers, pair_of):
    """The molecules F . payload . R that trimReads expects: original i framed by primer pair pair_of[i] (or by pair pair_of when
    that is one number) of primers = [(F, R), ...], both as they appear on the forward strand.  -> a list of base-code arrays."""
    if isinstance(pair_of, int):
        pair_of = [pair_of] * len(originals)
    if len(pair_of) != len(originals):
        raise ValueError("pair_of must name a primer pair per original")
    return [np.concatenate([_tokens(primers[k][0]), _tokens(o), _tokens(primers[k][1])]).astype(np.int8)
            for o, k in zip(originals, pair_of)]


def clusterSketch(reads, k=12, sketch=32):
    """dnas_cluster_sketch_host: the min-hash signatures clusterReads compares, uint32[N, sketch]."""
    reads = [_tokens(r) for r in reads]
    seqs, off = _concat(reads)
    sig = np.zeros((max(len(reads), 1), int(sketch)), dtype=np.uint32)
    _l.check(_l.lib().dnas_cluster_sketch_host(int(k), int(sketch), len(reads), seqs.ctypes.data, off.ctypes.data, sig.ctypes.data))
    return sig[:len(reads)]


def clusterCandidates(params, reads, band=32, k=12, sketch=32, min_shared=2):
    """dnas_cluster_candidates_host: the pairs clusterReads scores, in (i, j) order, and both item scores of each (read j as
    given, and its reverse complement, as a mutated copy of read i) -> (ij int64[C, 2], scores float64[C, 2]).  No GPU."""
    reads = [_tokens(r) for r in reads]
    seqs, off = _concat(reads)
    ij, scores, n_cand = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int64()
    _l.check(_l.lib().dnas_cluster_candidates_host(ctypes.byref(params.c), int(band), int(k), int(sketch), int(min_shared), len(reads),
                                                   seqs.ctypes.data, off.ctypes.data, ctypes.byref(ij), ctypes.byref(scores),
                                                   ctypes.byref(n_cand)))
    nc = n_cand.value
    return _take(ij, ctypes.c_int64, 2 * nc, np.int64).reshape(nc, 2), _take(scores, ctypes.c_double, 2 * nc, np.float64).reshape(nc, 2)


def paramsJSON(params):
    buf = ctypes.create_string_buffer(4096)
    _l.check(_l.lib().dnas_mutator_params_json(ctypes.byref(params.c), buf, 4096))
    return buf.value.decode()


def countsJSON(counts, n_len):
    c = np.ascontiguousarray(counts, dtype=np.float64)
    buf = ctypes.create_string_buffer(8192)
    _l.check(_l.lib().dnas_mutator_counts_json(c.ctypes.data, int(n_len), buf, 8192))
    return buf.value.decode()


def _stats_dict(st):
    return {k: (_stats_dict(getattr(st, k)) if isinstance(getattr(st, k), ctypes.Structure) else getattr(st, k)) for k, _ in st._fields_}


def rsEncode(data, n, k, device=0, host=False):
    """dnas_rs_encode: the systematic Reed-Solomon code over GF(2^8) (0x11d, alpha = 2) across the strands of a block.  data:
    uint8[B, k, L] (or [k, L]: one block), the data strands; -> uint8[B, n, L] ([n, L]), the strands 0 .. k-1 as given and the
    n - k parity strands, column j of a block a codeword.  On the GPU (device=-1: every GPU of the node), or with host=True the
    long division on the host (dnas_rs_encode_host)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    one = data.ndim == 2
    if one:
        data = data[None]
    if data.ndim != 3 or data.shape[1] != k:
        raise ValueError("data must be uint8[B, k, L]")
    B, L = data.shape[0], data.shape[2]
    out = np.zeros((B, n, L), dtype=np.uint8)
    if host:
        _l.check(_l.lib().dnas_rs_encode_host(int(n), int(k), L, B, data.ctypes.data, out.ctypes.data))
    else:
        _l.check(_l.lib().dnas_rs_encode(int(n), int(k), L, B, data.ctypes.data, out.ctypes.data, None, int(device)))
    return out[0] if one else out


class RsDecode:
    """What rsDecode returns: .blocks uint8[B, n, L] (the decoded blocks; a failed column holds what was received, 0 at erased
    positions), .status uint8[B, L] (dnas.lib.RS_*), .errors uint8[B, L] (present positions changed, 0 for a failed column),
    .fixed int32[B, n] (the corrected columns in which present strand p was changed); .stats: dnas_rs_stats of the call (None
    with host=True)."""

    def __init__(self, blocks, status, errors, fixed, stats):
        self.blocks, self.status, self.errors, self.fixed, self.stats = blocks, status, errors, fixed, stats


def rsDecode(blocks, present, n, k, device=0, host=False):
    """dnas_rs_decode: errors and erasures.  blocks: uint8[B, n, L]; present: uint8[B, n], 0 where the strand is an erasure (what
    is stored there is never read into the answer).  A column with f erasures comes back as the one codeword within e errors of
    it, 2 e + f <= n - k, if there is one; else it failed.  On the GPU (device=-1: every GPU of the node), or with host=True the
    statement on the host (dnas_rs_decode_host).  -> RsDecode."""
    blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
    present = np.ascontiguousarray(present, dtype=np.uint8)
    if blocks.ndim != 3 or blocks.shape[1] != n or present.shape != blocks.shape[:2]:
        raise ValueError("blocks must be uint8[B, n, L] and present uint8[B, n]")
    B, L = blocks.shape[0], blocks.shape[2]
    out = np.zeros((B, n, L), dtype=np.uint8)
    status, errors = np.zeros((B, L), dtype=np.uint8), np.zeros((B, L), dtype=np.uint8)
    fixed = np.zeros((B, n), dtype=np.int32)
    args = [int(n), int(k), L, B, blocks.ctypes.data, present.ctypes.data, out.ctypes.data, status.ctypes.data, errors.ctypes.data,
            fixed.ctypes.data]
    stats = None
    if host:
        _l.check(_l.lib().dnas_rs_decode_host(*args))
    else:
        st = _l.RsStatsC()
        _l.check(_l.lib().dnas_rs_decode(*args, ctypes.byref(st), int(device)))
        stats = _stats_dict(st)
    return RsDecode(out, status, errors, fixed, stats)


class OuterDecode:
    """What OuterCode.decode returns: .data (bytes: the file; the raw stream when .status is OUTER_NO_LENGTH or
    OUTER_BAD_LENGTH), .status (dnas.lib.OUTER_*), .present uint8[B, n] (0: the slot was an erasure), .column_status uint8[B, L]
    (dnas.lib.RS_*), .fixed int32[B, n] (columns in which the strand was corrected: which strands arrived wrong),
    .failed_ranges (a list of (begin, end) in the coordinates of .data: bytes that lie in failed columns), .stats:
    dnas_outer_stats of the call."""

    def __init__(self, data, status, present, column_status, fixed, failed_ranges, stats):
        self.data, self.status, self.present, self.column_status = data, status, present, column_status
        self.fixed, self.failed_ranges, self.stats = fixed, failed_ranges, stats


class OuterCode:
    """The outer code of a pool: RS(n, k) across blocks of n strands with bodies of body_len bytes, a record per strand (3 bytes
    of strand number, a CRC-8, the body: body_len + 4 bytes, what the inner code carries), a file as a stream over the data
    strands (dnas_outer_encode / dnas_outer_decode)."""

    def __init__(self, n, k, body_len):
        self.n, self.k, self.body_len = int(n), int(k), int(body_len)
        self.record_len = self.body_len + 4

    def n_blocks(self, length):
        return int(_l.lib().dnas_outer_blocks(int(length), self.k, self.body_len))

    def frame(self, s, body):
        """The record of strand number s with this body."""
        body = bytes(body)
        if len(body) != self.body_len:
            raise ValueError("a body has %d bytes" % self.body_len)
        out = ctypes.create_string_buffer(self.record_len)
        _l.check(_l.lib().dnas_outer_frame(int(s), body, self.body_len, out))
        return out.raw

    def encode(self, data, device=0, host=False):
        """-> (records, n_blocks): the n_blocks * n records of the file, in strand order."""
        data = bytes(data)
        p, nb = ctypes.c_void_p(), ctypes.c_int64()
        _l.check(_l.lib().dnas_outer_encode(data, len(data), self.n, self.k, self.body_len, int(device), int(bool(host)), ctypes.byref(nb),
                                            ctypes.byref(p)))
        raw = ctypes.string_at(p, nb.value * self.n * self.record_len)
        _l.lib().dnas_free(p)
        return [raw[i:i + self.record_len] for i in range(0, len(raw), self.record_len)], nb.value

    def decode(self, records, n_blocks, weights=None, device=0, host=False):
        """records: a pool of byte strings in any order, with duplicates, damaged ones and ones of another length; weights: None or
        one number per record.  -> OuterDecode."""
        records = [bytes(r) for r in records]
        if weights is not None and len(weights) != len(records):
            raise ValueError("weights must hold one value per record")
        raw = np.frombuffer(b"".join(records) + b"\0", dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.int64)
        w = None if weights is None else np.ascontiguousarray(np.append(np.asarray(weights, dtype=np.float64), 0.))
        B = int(n_blocks)
        present, fixed = np.zeros((max(B, 1), self.n), dtype=np.uint8), np.zeros((max(B, 1), self.n), dtype=np.int32)
        colst = np.zeros((max(B, 1), self.body_len), dtype=np.uint8)
        p, n, status, rp, nr, st = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_int32(), ctypes.c_void_p(), ctypes.c_int64(), _l.OuterStatsC()
        _l.check(_l.lib().dnas_outer_decode(len(records), raw.ctypes.data, off.ctypes.data, None if w is None else w.ctypes.data, self.n,
                                            self.k, self.body_len, B, int(device), int(bool(host)), ctypes.byref(p), ctypes.byref(n),
                                            ctypes.byref(status), present.ctypes.data, colst.ctypes.data, fixed.ctypes.data, ctypes.byref(rp),
                                            ctypes.byref(nr), ctypes.byref(st)))
        data = ctypes.string_at(p, n.value)
        flat = np.ctypeslib.as_array(ctypes.cast(rp, ctypes.POINTER(ctypes.c_int64)), shape=(max(2 * nr.value, 1),))[:2 * nr.value].copy()
        _l.lib().dnas_free(p)
        _l.lib().dnas_free(rp)
        ranges = [(int(a), int(b)) for a, b in flat.reshape(-1, 2)]
        return OuterDecode(data, status.value, present[:B], colst[:B], fixed[:B], ranges, _stats_dict(st))

    def decode_messages(self, symbol_strings, n_blocks, weights=None, device=0, host=False):
        """The same from decoded messages: symbol strings ('0' / '1', as ViterbiDecoder.decode returns them), each through
        symbolsToBytes, or a ClusterDecodes, whose .symbols are taken and whose .confidence (score="forward") are the weights
        unless weights are given.  An empty message is no record."""
        if hasattr(symbol_strings, "symbols"):
            if weights is None and hasattr(symbol_strings, "confidence"):
                weights = symbol_strings.confidence
            symbol_strings = symbol_strings.symbols
        records = [symbolsToBytes(s) if len(s) else b"" for s in symbol_strings]
        return self.decode(records, n_blocks, weights=weights, device=device, host=host)


def debugAllocStats(reset=False):
    """What the debug allocation mode (DNAS_DEBUG_ALLOC=<byte>, a testing aid) has seen: guarded allocations made, guarded frees
    checked, guard bands found changed, and of the first such block its bytes and the offset of the first changed byte."""
    out = (ctypes.c_int64 * 5)()
    _l.check(_l.lib().dnas_debug_alloc_stats(out, int(bool(reset))))
    return dict(zip(("allocations", "frees_checked", "violations", "first_bytes", "first_offset"), (int(v) for v in out)))


def symbolsToBytes(symbols):
    """BinaryWriter (decoder.h:193-240): '0'/'1' symbols -> bytes, LSB first; other symbols ignored."""
    b = symbols.encode() if isinstance(symbols, str) else symbols
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    _l.check(_l.lib().dnas_symbols_to_bytes(b, len(b), ctypes.byref(p), ctypes.byref(n)))
    out = ctypes.string_at(p, n.value)
    _l.lib().dnas_free(p)
    return out
