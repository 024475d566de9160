"""PskContext: numpy-level wrapper over the C ABI (one context = one GPU = one rank)."""
import ctypes
import os

import numpy as np

from . import _lib
from ._lib import PskError


def words_per_row(n_samples):
    """u64 words per presence row: 1 up to 64 samples, else ceil(n/64) rounded up to even (rows are 16-byte aligned)."""
    w = (n_samples + 63) // 64
    return 1 if w <= 1 else (w + 1) & ~1


def _ptr(a):
    return None if a is None else a.ctypes.data


def pack_strings(strings):
    """ACGT strings in the layout of psk_asm_round: (words, word_off[n], len_bases[n]) -- 32 bases per u64, the first base in
    the two most significant bits, every string from a word of its own."""
    lens = np.array([len(s) for s in strings], dtype=np.uint32)
    nw = (lens.astype(np.int64) + 31) // 32
    word_off = np.zeros(len(strings), dtype=np.uint64)
    if len(strings) > 1:
        word_off[1:] = np.cumsum(nw[:-1])
    codes = np.zeros(int(nw.sum()) * 32, dtype=np.uint64)
    lut = np.full(256, 255, dtype=np.uint8)
    for ch, v in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3) * 2):
        lut[ch] = v
    for s, off in zip(strings, word_off):
        c = lut[np.frombuffer(s.encode("ascii"), dtype=np.uint8)]
        if (c == 255).any():
            raise ValueError("not a string of bases: %r" % s[:40])
        codes[int(off) * 32: int(off) * 32 + len(s)] = c
    shifts = (np.uint64(62) - np.arange(32, dtype=np.uint64) * np.uint64(2))
    words = np.bitwise_or.reduce(codes.reshape(-1, 32) << shifts[None, :], axis=1) if len(codes) else np.zeros(0, dtype=np.uint64)
    return np.ascontiguousarray(words, dtype=np.uint64), word_off, lens


def _file_size(path):
    try:
        return os.stat(path).st_size
    except OSError:
        return 0


class PskContext:
    def __init__(self, device=0):
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self._lib.psk_init(int(device), ctypes.byref(h))
        if rc != 0:
            raise PskError("psk_init(%d) failed: %s" % (device, self._lib.psk_last_error(None).decode()), code=rc)
        self._h = h
        self.device = device
        self.k = None
        self.n_samples = None

    # -- plumbing -------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise PskError("%s failed (%d): %s" % (what, rc, self._lib.psk_last_error(self._h).decode()), code=rc)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.psk_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        ncu = ctypes.c_int()
        mem = ctypes.c_uint64()
        self._check(self._lib.psk_device_info(self._h, name, 256, ctypes.byref(ncu), ctypes.byref(mem)), "device_info")
        return {"name": name.value.decode(), "n_cu": ncu.value, "hbm_bytes": mem.value}

    # -- k-mer plane ----------------------------------------------------------------------------
    def begin(self, k, n_samples, slab_lo=0, slab_hi=0):
        self._check(self._lib.psk_begin(self._h, int(k), int(n_samples), int(slab_lo), int(slab_hi)), "psk_begin")
        self.k, self.n_samples = int(k), int(n_samples)

    def count_kmers(self, sample_idx, data):
        data = bytes(data)
        nu, nt = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.psk_count_kmers(self._h, int(sample_idx), data, len(data), ctypes.byref(nu),
                                              ctypes.byref(nt)), "psk_count_kmers")
        return nu.value, nt.value

    def count_kmers_batch(self, first_idx, datas, n_threads=4, sketch=None):
        """Counts several samples in one call; host tokenisation runs ahead on n_threads threads.
        sketch=(k, size, seed): also returns every sample's MinHash sketch (third element: list of uint64 arrays),
        computed from the clean stream that is on the device for counting anyway."""
        datas = [bytes(d) for d in datas]
        n = len(datas)
        arr = (ctypes.c_char_p * n)(*datas)
        lens = (ctypes.c_size_t * n)(*[len(d) for d in datas])
        nu = np.zeros(n, dtype=np.uint64)
        nt = np.zeros(n, dtype=np.uint64)
        if sketch is None:
            self._check(self._lib.psk_count_kmers_batch(self._h, int(first_idx), n, arr, lens, _ptr(nu), _ptr(nt),
                                                        int(n_threads)), "psk_count_kmers_batch")
            return nu.astype(np.int64).tolist(), nt.astype(np.int64).tolist()
        k, size, seed = sketch
        hashes = np.zeros((n, int(size)), dtype=np.uint64)
        nh = np.zeros(n, dtype=np.uint64)
        self._check(self._lib.psk_count_kmers_batch_sketch(self._h, int(first_idx), n, arr, lens, _ptr(nu), _ptr(nt),
                                                           int(n_threads), int(k), int(size), int(seed), _ptr(hashes),
                                                           _ptr(nh)), "psk_count_kmers_batch_sketch")
        return (nu.astype(np.int64).tolist(), nt.astype(np.int64).tolist(),
                [hashes[i, : int(nh[i])].copy() for i in range(n)])

    def count_kmers_files(self, first_idx, paths, n_threads=4, sketch=None):
        """count_kmers_batch for UNCOMPRESSED files: the library's framing threads read them (psk_count_kmers_files).
        Returns (n_unique, n_total[, sketches])."""
        enc = [os.fsencode(p) for p in paths]
        n = len(enc)
        arr = (ctypes.c_char_p * n)(*enc)
        sizes = (ctypes.c_size_t * n)(*[_file_size(p) for p in paths])
        nu = np.zeros(n, dtype=np.uint64)
        nt = np.zeros(n, dtype=np.uint64)
        k, size, seed = sketch if sketch is not None else (0, 1, 0)
        hashes = np.zeros((n, int(size)), dtype=np.uint64) if sketch is not None else None
        nh = np.zeros(n, dtype=np.uint64) if sketch is not None else None
        self._check(self._lib.psk_count_kmers_files(self._h, int(first_idx), n, arr, sizes, _ptr(nu), _ptr(nt), int(n_threads),
                                                    int(k), int(size), int(seed), _ptr(hashes), _ptr(nh)),
                    "psk_count_kmers_files")
        out = (nu.astype(np.int64).tolist(), nt.astype(np.int64).tolist())
        if sketch is not None:
            out += ([hashes[i, : int(nh[i])].copy() for i in range(n)],)
        return out

    def get_list(self, sample_idx, n_unique):
        words = np.empty(n_unique, dtype=np.uint64)
        freqs = np.empty(n_unique, dtype=np.uint32)
        self._check(self._lib.psk_get_list(self._h, int(sample_idx), _ptr(words), _ptr(freqs), n_unique), "psk_get_list")
        return words, freqs

    def gz_inflate(self, images, want_text=True, per_file=False):
        """The text of gzip images, inflated on the device (csrc/gz_inflate.hip).  Returns (texts or None, lengths, routes,
        device_ms); routes: 1 device, 2 device (BGZF), 0 zlib on the host.  want_text=False: lengths only (measurements).
        A file zlib refuses raises PskError (zlib's words) -- per_file=True instead returns route -1 and text None for it."""
        images = [bytes(b) for b in images]
        n = len(images)
        ptrs = (ctypes.c_char_p * max(n, 1))(*images)
        sizes = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in images])
        lens = np.zeros(max(n, 1), dtype=np.uint64)
        route = np.zeros(max(n, 1), dtype=np.int32)
        ms = ctypes.c_double()

        def call(outp, caps):
            route[:] = 0
            rc = self._lib.psk_gz_inflate(self._h, n, ptrs, sizes, outp, caps, _ptr(lens), _ptr(route), ctypes.byref(ms))
            if not (per_file and rc == -1 and (route[:n] == -1).any()):     # PSK_EINVAL with the refused files marked
                self._check(rc, "psk_gz_inflate")
        call(None, None)
        if not want_text:
            return None, lens[:n].tolist(), route[:n].tolist(), ms.value
        bufs = [np.empty(max(int(l), 1), dtype=np.uint8) for l in lens[:n]]
        outp = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        caps = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bufs])
        call(outp, caps)
        return ([None if r == -1 else b[:int(l)].tobytes() for b, l, r in zip(bufs, lens[:n], route[:n])], lens[:n].tolist(),
                route[:n].tolist(), ms.value)

    # -- multi-GPU ingest: slab ranges of sorted lists (dist.ListExchange) ---------------------------
    def lists_split(self, first_idx, n, bounds):
        """offsets[i][b] = number of words of sample first_idx + i below bounds[b] (a 0 after the first bound = end)."""
        b = np.ascontiguousarray(bounds, dtype=np.uint64)
        out = np.zeros((int(n), len(b)), dtype=np.uint64)
        self._check(self._lib.psk_lists_split(self._h, int(first_idx), int(n), _ptr(b), len(b), _ptr(out)), "psk_lists_split")
        return out.astype(np.int64)

    def copy_list_ranges(self, sample_idx, start, count, dev_words_ptr, dev_freqs_ptr):
        """Ranges [start[r], start[r] + count[r]) of the lists sample_idx[r], packed back to back into DEVICE buffers
        given as raw pointers (torch's data_ptr())."""
        si = np.ascontiguousarray(sample_idx, dtype=np.int32)
        st = np.ascontiguousarray(start, dtype=np.uint64)
        ct = np.ascontiguousarray(count, dtype=np.uint64)
        self._check(self._lib.psk_copy_list_ranges(self._h, len(si), _ptr(si), _ptr(st), _ptr(ct), ctypes.c_void_p(dev_words_ptr),
                                                   ctypes.c_void_p(dev_freqs_ptr)), "psk_copy_list_ranges")

    def release_lists(self):
        """Gives the device memory of the lists back; every sample is "not counted" again."""
        self._check(self._lib.psk_release_lists(self._h), "psk_release_lists")

    def set_lists_device(self, sample_idx, count, n_total, dev_words_ptr, dev_freqs_ptr):
        """Installs len(sample_idx) lists held back to back in DEVICE memory as the lists of those samples."""
        si = np.ascontiguousarray(sample_idx, dtype=np.int32)
        ct = np.ascontiguousarray(count, dtype=np.uint64)
        tot = np.ascontiguousarray(n_total, dtype=np.uint64)
        self._check(self._lib.psk_set_lists_device(self._h, len(si), _ptr(si), _ptr(ct), _ptr(tot), ctypes.c_void_p(dev_words_ptr),
                                                   ctypes.c_void_p(dev_freqs_ptr)), "psk_set_lists_device")

    def lookup_counts(self, sample_idx, words):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        out = np.zeros(len(words), dtype=np.uint32)
        self._check(self._lib.psk_lookup_counts(self._h, int(sample_idx), _ptr(words), len(words), _ptr(out)),
                    "psk_lookup_counts")
        return out

    def build_presence(self):
        m = ctypes.c_uint64()
        self._check(self._lib.psk_build_presence(self._h, ctypes.byref(m)), "psk_build_presence")
        return m.value

    def presence_shape(self):
        m, w, n = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.psk_presence_shape(self._h, ctypes.byref(m), ctypes.byref(w), ctypes.byref(n)),
                    "psk_presence_shape")
        return m.value, w.value, n.value

    def get_union(self):
        m, _, _ = self.presence_shape()
        words = np.empty(m, dtype=np.uint64)
        self._check(self._lib.psk_get_union(self._h, _ptr(words), m), "psk_get_union")
        return words

    def get_rows(self, row_idx):
        row_idx = np.ascontiguousarray(row_idx, dtype=np.uint64)
        _, wpr, _ = self.presence_shape()
        out = np.zeros((len(row_idx), wpr), dtype=np.uint64)
        self._check(self._lib.psk_get_rows(self._h, _ptr(row_idx), len(row_idx), _ptr(out)), "psk_get_rows")
        return out

    def intersect_db(self, db_words):
        db = np.ascontiguousarray(np.unique(np.asarray(db_words, dtype=np.uint64)))
        m = ctypes.c_uint64()
        self._check(self._lib.psk_intersect_db(self._h, _ptr(db), len(db), ctypes.byref(m)), "psk_intersect_db")
        return m.value

    def set_presence(self, bits, n_samples, words=None):
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        m, wpr = bits.shape
        if words is not None:
            words = np.ascontiguousarray(words, dtype=np.uint64)
        self._check(self._lib.psk_set_presence(self._h, _ptr(words), _ptr(bits), m, wpr, int(n_samples)),
                    "psk_set_presence")
        self.n_samples = int(n_samples)

    def synth_presence(self, n_kmers, n_samples, seed=1):
        self._check(self._lib.psk_synth_presence(self._h, int(n_kmers), int(n_samples), int(seed)), "psk_synth_presence")
        self.n_samples = int(n_samples)

    # -- association scans ----------------------------------------------------------------------
    def chi2_scan(self, pheno, weights, min_samples, max_samples, pvalue_cutoff, omit_B, n_kmers_global=0):
        """pheno: int8 array, 1 / 0 / -1 (NA).  Returns the number of surviving k-mers."""
        ph = np.ascontiguousarray(pheno, dtype=np.int8)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        n = ctypes.c_uint64()
        self._check(self._lib.psk_chi2_scan(self._h, _ptr(ph), _ptr(w), int(min_samples), int(max_samples),
                                            float(pvalue_cutoff), int(bool(omit_B)), int(n_kmers_global),
                                            ctypes.byref(n)), "psk_chi2_scan")
        return n.value

    def chi2_scan_begin(self, pheno, weights, min_samples, max_samples, pvalue_cutoff, omit_B, n_kmers_global=0):
        """Launches the scan and returns at once; scan_end() waits for it (psk_chi2_scan_begin / psk_scan_end)."""
        ph = np.ascontiguousarray(pheno, dtype=np.int8)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        self._check(self._lib.psk_chi2_scan_begin(self._h, _ptr(ph), _ptr(w), int(min_samples), int(max_samples),
                                                  float(pvalue_cutoff), int(bool(omit_B)), int(n_kmers_global)),
                    "psk_chi2_scan_begin")

    def scan_end(self):
        n = ctypes.c_uint64()
        self._check(self._lib.psk_scan_end(self._h, ctypes.byref(n)), "psk_scan_end")
        return n.value

    def ttest_scan(self, values, valid, weights, min_samples, max_samples, pvalue_cutoff, n_kmers_global=0):
        v = np.ascontiguousarray(values, dtype=np.float64)
        ok = np.ascontiguousarray(valid, dtype=np.uint8)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        n = ctypes.c_uint64()
        self._check(self._lib.psk_ttest_scan(self._h, _ptr(v), _ptr(ok), _ptr(w), int(min_samples), int(max_samples),
                                             float(pvalue_cutoff), int(n_kmers_global), ctypes.byref(n)),
                    "psk_ttest_scan")
        return n.value

    def get_results(self, n_pass):
        n = int(n_pass)
        out = {"row": np.zeros(n, np.uint64), "word": np.zeros(n, np.uint64), "stat": np.zeros(n), "p": np.zeros(n),
               "mean_x": np.zeros(n), "mean_y": np.zeros(n), "n_with": np.zeros(n, np.int32)}
        self._check(self._lib.psk_get_results(self._h, _ptr(out["row"]), _ptr(out["word"]), _ptr(out["stat"]),
                                              _ptr(out["p"]), _ptr(out["mean_x"]), _ptr(out["mean_y"]),
                                              _ptr(out["n_with"]), n), "psk_get_results")
        return out

    def export_survivors(self, device_ptr, cap_records):
        """Packs the last scan's survivors into a caller DEVICE buffer (see psk_export_survivors)."""
        n = ctypes.c_uint64()
        self._check(self._lib.psk_export_survivors(self._h, ctypes.c_void_p(int(device_ptr)), int(cap_records),
                                                   ctypes.byref(n)), "psk_export_survivors")
        return n.value

    def export_survivors_async(self, device_ptr, cap_records, stream_handle):
        """psk_export_survivors_async: the export is queued on `stream_handle` (a hipStream_t as an integer) and
        not waited for.  The number of records is the n_pass the scan returned."""
        self._check(self._lib.psk_export_survivors_async(self._h, ctypes.c_void_p(int(device_ptr)), int(cap_records),
                                                         ctypes.c_void_p(int(stream_handle))), "psk_export_survivors_async")

    # -- multi-GPU collectives (RCCL, comm.hip) and plain device buffers ---------------------------
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        n = self._lib.psk_comm_unique_id(self._h, buf, 128)
        if n < 0:
            self._check(n, "psk_comm_unique_id")
        return buf.raw[:n]

    def comm_init(self, uid, rank, world):
        self._check(self._lib.psk_comm_init(self._h, bytes(uid), len(uid), int(rank), int(world)), "psk_comm_init")

    def comm_size(self):
        """ncclCommCount of this context's communicator."""
        n = self._lib.psk_comm_size(self._h)
        if n < 0:
            self._check(n, "psk_comm_size")
        return n

    def comm_stream(self):
        return self._lib.psk_comm_stream(self._h) or 0

    def comm_sync(self):
        self._check(self._lib.psk_comm_sync(self._h), "psk_comm_sync")

    def comm_allreduce(self, arr, op="sum"):
        """In place on a contiguous uint64 or float64 array."""
        assert arr.dtype in (np.uint64, np.float64) and arr.flags.c_contiguous
        self._check(self._lib.psk_comm_allreduce(self._h, _ptr(arr), arr.size, 0 if arr.dtype == np.uint64 else 1,
                                                 {"sum": 0, "max": 1}[op]), "psk_comm_allreduce")
        return arr

    def comm_allgather_host(self, send, world):
        send = np.ascontiguousarray(send).view(np.uint8).ravel()
        recv = np.empty((world, send.size), dtype=np.uint8)
        self._check(self._lib.psk_comm_allgather_host(self._h, _ptr(send), _ptr(recv), send.size), "psk_comm_allgather_host")
        return recv

    def comm_allgather_device(self, send_ptr, recv_ptr, nbytes):
        self._check(self._lib.psk_comm_allgather_device(self._h, ctypes.c_void_p(int(send_ptr)), ctypes.c_void_p(int(recv_ptr)),
                                                        int(nbytes)), "psk_comm_allgather_device")

    def comm_alltoallv_device(self, send_ptr, send_counts, recv_ptr, recv_counts, elem_bytes):
        sc = np.ascontiguousarray(send_counts, dtype=np.uint64)
        rc = np.ascontiguousarray(recv_counts, dtype=np.uint64)
        self._check(self._lib.psk_comm_alltoallv_device(self._h, ctypes.c_void_p(int(send_ptr)), _ptr(sc),
                                                        ctypes.c_void_p(int(recv_ptr)), _ptr(rc), int(elem_bytes)),
                    "psk_comm_alltoallv_device")

    def dev_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._check(self._lib.psk_dev_alloc(self._h, int(nbytes), ctypes.byref(p)), "psk_dev_alloc")
        return p.value

    def dev_free(self, ptr):
        if ptr and getattr(self, "_h", None):
            self._check(self._lib.psk_dev_free(self._h, ctypes.c_void_p(int(ptr))), "psk_dev_free")

    def dev_download(self, ptr, nbytes, behind_collectives=False):
        out = np.empty(int(nbytes), dtype=np.uint8)
        self._check(self._lib.psk_dev_copy(self._h, _ptr(out), ctypes.c_void_p(int(ptr)), int(nbytes), 1,
                                           1 if behind_collectives else 0), "psk_dev_copy")
        return out

    def dev_upload(self, ptr, arr):
        a = np.ascontiguousarray(arr)
        self._check(self._lib.psk_dev_copy(self._h, ctypes.c_void_p(int(ptr)), _ptr(a), a.nbytes, 0, 0), "psk_dev_copy")

    def compact_info(self):
        """(has the matrix an exception-coded copy for the unweighted chi2 scan, rows of its dense side matrix)"""
        enc, n_ov = ctypes.c_int(), ctypes.c_uint64()
        self._check(self._lib.psk_compact_info(self._h, ctypes.byref(enc), ctypes.byref(n_ov)), "psk_compact_info")
        return bool(enc.value), n_ov.value

    def last_scan_plan(self):
        """(the last chi2 scan took the exception-coded path, its class mask, it left the slot stream unread):
        psk_last_scan_plan"""
        enc, mask, skipped = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_int()
        self._check(self._lib.psk_last_scan_plan(self._h, ctypes.byref(enc), ctypes.byref(mask), ctypes.byref(skipped)),
                    "psk_last_scan_plan")
        return bool(enc.value), mask.value, bool(skipped.value)

    def last_scan_filter(self):
        """(the last chi2 scan ran the popcount-filtered side-matrix kernel, overflow rows whose popcount its plan
        leaves, overflow rows): psk_last_scan_filter"""
        filt, feas, n_ov = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.psk_last_scan_filter(self._h, ctypes.byref(filt), ctypes.byref(feas), ctypes.byref(n_ov)),
                    "psk_last_scan_filter")
        return bool(filt.value), feas.value, n_ov.value

    def last_scan_form(self):
        """Kernel form of the last chi2 scan set up (psk_last_scan_form): one of SCAN_FORMS"""
        form = ctypes.c_int()
        self._check(self._lib.psk_last_scan_form(self._h, ctypes.byref(form)), "psk_last_scan_form")
        return SCAN_FORMS[form.value] if form.value >= 0 else None

    def cx_pc_index(self):
        """(positions of the side-matrix rows grouped by popcount, u32 [n_ov]; starts of the buckets, u64 [n_samples + 2]):
        the encoder's index as the device holds it (psk_cx_pc_index; tests)"""
        enc, n_ov = self.compact_info()
        index, start = np.zeros(max(n_ov, 1), np.uint32), np.zeros(self.n_samples + 2, np.uint64)
        self._check(self._lib.psk_cx_pc_index(self._h, _ptr(index), n_ov, _ptr(start), len(start)), "psk_cx_pc_index")
        return index[:n_ov], start

    def last_scan_ms(self):
        return self._lib.psk_last_scan_ms(self._h)

    def rescan_timed(self, reps):
        ms = ctypes.c_double()
        self._check(self._lib.psk_rescan_timed(self._h, int(reps), ctypes.byref(ms)), "psk_rescan_timed")
        return ms.value

    def rescan_times(self, reps):
        """HIP-event duration in ms of each of `reps` repeats of the last chi2 scan (psk_rescan_times)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        self._check(self._lib.psk_rescan_times(self._h, int(reps), _ptr(ms)), "psk_rescan_times")
        return ms

    def stream_read_ceiling(self, reps):
        """(mean ms, bytes, shape) of the fastest plain 16-B-per-lane read of the presence matrix: the stream-read ceiling
        the scan's achieved bandwidth is quoted against (psk_stream_read_ceiling)."""
        ms, nb, shape = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_int()
        self._check(self._lib.psk_stream_read_ceiling(self._h, int(reps), ctypes.byref(ms), ctypes.byref(nb), ctypes.byref(shape)),
                    "psk_stream_read_ceiling")
        return ms.value, nb.value, ("grid-stride, non-temporal", "grid-stride", "wave-contiguous, non-temporal", "wave-contiguous")[shape.value]

    # -- models -----------------------------------------------------------------------------------
    @staticmethod
    def _fit_arrays(X, y, ydtype, fold, fit_param, fit_fold):
        """(X, n, p, y, fold, fit_param, fit_fold, n_fits) as the fit entry points take them: contiguous, in the ABI's types."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        fit_param = np.ascontiguousarray(fit_param, dtype=np.float64)
        return (X, X.shape[0], X.shape[1], np.ascontiguousarray(y, dtype=ydtype), np.ascontiguousarray(fold, dtype=np.int32), fit_param,
                np.ascontiguousarray(fit_fold, dtype=np.int32), len(fit_param))

    def _fit(self, fn, name, X, y, ydtype, fold, fit_param, fit_fold, *extra):
        """A linear-model entry point: (coef[n_fits][p], intercept[n_fits], iterations[n_fits]); `extra`: the arguments
        it takes between n_fits and the outputs."""
        X, n, p, y, fold, fit_param, fit_fold, nf = self._fit_arrays(X, y, ydtype, fold, fit_param, fit_fold)
        coef, icpt, iters = np.zeros((nf, p)), np.zeros(nf), np.zeros(nf, dtype=np.int32)
        self._check(fn(self._h, _ptr(X), _ptr(y), n, p, _ptr(fold), _ptr(fit_param), _ptr(fit_fold), nf, *extra, _ptr(coef), _ptr(icpt),
                       _ptr(iters)), name)
        return coef, icpt, iters

    def logreg_l1_fit(self, X, y01, fold, fit_param, fit_fold, tol=1e-4, max_iter=1000):
        return self._fit(self._lib.psk_logreg_l1_fit, "psk_logreg_l1_fit", X, y01, np.int32, fold, fit_param, fit_fold,
                         float(tol), int(max_iter))

    def logreg_l1_free_fit(self, X, y01, fold, fit_param, fit_fold, tol=1e-4, max_iter=1000):
        """L1 logistic fits with a free intercept (psk_logreg_l1_free_fit): the objective of scikit-learn's saga solver,
        ||w||_1 + C sum log(1 + exp(-y (w.x + b))), same batching, routes and knobs as logreg_l1_fit."""
        return self._fit(self._lib.psk_logreg_l1_free_fit, "psk_logreg_l1_free_fit", X, y01, np.int32, fold, fit_param, fit_fold,
                         float(tol), int(max_iter))

    def lasso_fit(self, X, y, fold, fit_param, fit_fold, tol=1e-4, max_iter=1000):
        return self._fit(self._lib.psk_lasso_fit, "psk_lasso_fit", X, y, np.float64, fold, fit_param, fit_fold, float(tol),
                         int(max_iter))

    def enet_fit(self, X, y, fold, fit_alpha, fit_fold, l1_ratio=0.5, tol=1e-4, max_iter=1000):
        """Elastic-net fits (psk_enet_fit): same batching and routes as lasso_fit, one l1_ratio in [0, 1] for the call."""
        return self._fit(self._lib.psk_enet_fit, "psk_enet_fit", X, y, np.float64, fold, fit_alpha, fit_fold, float(l1_ratio),
                         float(tol), int(max_iter))

    def ridge_fit(self, X, y, fold, fit_param, fit_fold):
        """Ridge fits (psk_ridge_fit): same batching as lasso_fit, solved to convergence."""
        return self._fit(self._lib.psk_ridge_fit, "psk_ridge_fit", X, y, np.float64, fold, fit_param, fit_fold)

    def logreg_l2_fit(self, X, y01, fold, fit_param, fit_fold, tol=1e-4, max_iter=1000, penalise_intercept=False):
        return self._fit(self._lib.psk_logreg_l2_fit, "psk_logreg_l2_fit", X, y01, np.int32, fold, fit_param, fit_fold,
                         float(tol), int(max_iter), int(bool(penalise_intercept)))

    def svc_fit(self, X, y01, fold, fit_C, fit_fold, kernel="linear", fit_gamma=None, tol=1e-3, max_iter=-1):
        """C-SVC fits (psk_svc_fit): libsvm's solver without shrinking, one workgroup per fit.  Returns
        (dual[n_fits][n], rho[n_fits], dec[n_fits][n], iters[n_fits]) in libsvm's sign: class 0 is positive."""
        if kernel not in ("linear", "rbf"):
            raise ValueError("kernel must be 'linear' or 'rbf', got %r" % (kernel,))
        X, n, p, y, fold, fit_C, fit_fold, nf = self._fit_arrays(X, y01, np.int32, fold, fit_C, fit_fold)
        if kernel == "rbf":
            fit_gamma = np.ascontiguousarray(np.broadcast_to(np.asarray(fit_gamma, dtype=np.float64), (nf,)))
        dual, rho, dec = np.zeros((nf, n)), np.zeros(nf), np.zeros((nf, n))
        iters = np.zeros(nf, dtype=np.int32)
        self._check(self._lib.psk_svc_fit(self._h, _ptr(X), _ptr(y), n, p, _ptr(fold), _ptr(fit_C),
                                          _ptr(fit_gamma) if kernel == "rbf" else None, _ptr(fit_fold), nf,
                                          1 if kernel == "rbf" else 0, float(tol), int(max_iter), _ptr(dual), _ptr(rho),
                                          _ptr(dec), _ptr(iters)), "psk_svc_fit")
        return dual, rho, dec, iters

    def svc_decision(self, X, SV, coef, rho, kernel="linear", gamma=0.0):
        """Decision values of the rows X[m][p] under a fitted SVM (psk_svc_decision): (sum_j coef[j] K(SV[j], X[i])) - rho in
        libsvm's sign, the support vectors added one after the other as psk_svc_fit's own decision values are.  coef[n_sv]:
        y_j alpha_j (-dual_coef_[0]).  Returns dec[m]."""
        if kernel not in ("linear", "rbf"):
            raise ValueError("kernel must be 'linear' or 'rbf', got %r" % (kernel,))
        X = np.ascontiguousarray(X, dtype=np.float32)
        SV = np.ascontiguousarray(SV, dtype=np.float32)
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        if X.ndim != 2 or SV.ndim != 2 or X.shape[1] != SV.shape[1] or len(coef) != SV.shape[0]:
            raise ValueError("svc_decision: X[m][p], SV[n_sv][p] and coef[n_sv] do not fit together")
        dec = np.zeros(X.shape[0])
        self._check(self._lib.psk_svc_decision(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(SV), SV.shape[0], _ptr(coef), float(rho),
                                               1 if kernel == "rbf" else 0, float(gamma), _ptr(dec)), "psk_svc_decision")
        return dec

    TREE_NODE_CAP = 2047      # PSK_TREE_NODE_CAP of include/psk.h

    COUNT_MAX = 1 << 24       # the largest value of a count design (include/psk.h, f9)

    @staticmethod
    def _tree_dict(nodes, impurity, max_depth, leaf, threshold=None):
        """nodes[k][6] (feature, left, right, n_node_samples, the two class counts), impurity[k] by node in pre-order,
        the tree's depth and leaf[n], every sample's leaf, as the dictionary tree_fit and forest_fit return per tree; the
        count calls add threshold[k]."""
        d = dict(node_count=len(nodes), max_depth=int(max_depth), feature=nodes[:, 0].astype(np.int64), left=nodes[:, 1].astype(np.int64),
                 right=nodes[:, 2].astype(np.int64), n_node_samples=nodes[:, 3].astype(np.int64), counts=nodes[:, 4:6].astype(np.int64),
                 impurity=impurity.copy(), leaf=leaf.astype(np.int64))
        if threshold is not None:
            d["threshold"] = threshold.copy()
        return d

    @classmethod
    def _count_design(cls, X, who):
        """The float32 design of the count calls.  The range is checked on the float64 values: the cast would round
        2^24 + 1 to 2^24 and hide it."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2 or not np.all((X >= 0) & (X <= cls.COUNT_MAX) & (X == np.floor(X))):    # (a NaN fails every comparison)
            raise ValueError("%s takes a count design: every value must be an integer in 0 .. 2^24" % who)
        return np.ascontiguousarray(X, dtype=np.float32)

    def tree_fit(self, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        """Decision-tree fits (psk_tree_fit): scikit-learn's depth-first best-split builder on a 0/1 design, one workgroup
        per fit, the lowest column index among equally good splits.  fit_criterion: 0 / 'gini', 1 / 'entropy'.  Returns a
        list with one dict per fit: node_count, max_depth, feature / left / right / n_node_samples / counts[:, 2] /
        impurity by node (pre-order), and leaf[n], frac[n]: every sample's leaf and that leaf's class-1 fraction."""
        return self._tree_fit(False, np.ascontiguousarray(X, dtype=np.float32), y01, fold, fit_max_depth, fit_criterion, fit_fold)

    def tree_fit_counts(self, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        """tree_fit on a count design (psk_tree_fit_counts): integers in 0 .. 2^24, ValueError otherwise.  The same dicts
        plus threshold by node: scikit-learn's midpoint between the two values around the split among the node's training
        samples, -2 at a leaf; x <= threshold goes left."""
        return self._tree_fit(True, self._count_design(X, "tree_fit_counts"), y01, fold, fit_max_depth, fit_criterion, fit_fold)

    @staticmethod
    def _real_design(X, who):
        """The float32 design of the real calls: finite after the rounding to float32 (the library refuses the rest too)."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or not np.all(np.isfinite(X)):
            raise ValueError("%s takes a real-valued design: every value must be finite in float32" % who)
        return X

    def tree_fit_real(self, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        """tree_fit_counts on a design of any finite float32 values (psk_tree_fit_real), ValueError on a NaN or an infinity.
        The same dicts; any two different float32 values of a column make a candidate split, -0.0 and +0.0 are one value."""
        return self._tree_fit("real", self._real_design(X, "tree_fit_real"), y01, fold, fit_max_depth, fit_criterion, fit_fold)

    def _tree_fit(self, counts, X, y01, fold, fit_max_depth, fit_criterion, fit_fold):
        """counts: False (0/1 design), True (count design) or 'real' (any finite float32 values)."""
        n, p = X.shape
        y = np.ascontiguousarray(y01, dtype=np.int32)
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        depth = np.ascontiguousarray(fit_max_depth, dtype=np.int32)
        crit = np.ascontiguousarray([{"gini": 0, "entropy": 1}.get(c, c) for c in fit_criterion], dtype=np.int32)
        fit_fold = np.ascontiguousarray(fit_fold, dtype=np.int32)
        nf, cap = len(depth), self.TREE_NODE_CAP
        count, deepest = np.zeros(nf, dtype=np.int32), np.zeros(nf, dtype=np.int32)
        nodes, imp = np.zeros((nf, cap, 6), dtype=np.int32), np.zeros((nf, cap))
        leaf, frac = np.zeros((nf, n), dtype=np.int32), np.zeros((nf, n))
        args = (self._h, _ptr(X), _ptr(y), n, p, _ptr(fold), _ptr(depth), _ptr(crit), _ptr(fit_fold), nf, _ptr(count), _ptr(deepest),
                _ptr(nodes), _ptr(imp), _ptr(leaf), _ptr(frac))
        if not counts:
            self._check(self._lib.psk_tree_fit(*args), "psk_tree_fit")
            return [dict(self._tree_dict(nodes[j, :count[j]], imp[j, :count[j]], deepest[j], leaf[j]), frac=frac[j].copy()) for j in range(nf)]
        thr = np.zeros((nf, cap))
        name = "psk_tree_fit_real" if counts == "real" else "psk_tree_fit_counts"
        self._check(getattr(self._lib, name)(*args, _ptr(thr)), name)
        return [dict(self._tree_dict(nodes[j, :count[j]], imp[j, :count[j]], deepest[j], leaf[j], thr[j, :count[j]]), frac=frac[j].copy())
                for j in range(nf)]

    def forest_fit(self, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                   fit_min_samples_leaf, fit_min_samples_split, export=None):
        """Random-forest fits (psk_forest_fit): scikit-learn's forest trees for the draws the caller made, one workgroup per
        tree.  tree_weight[n_trees][n]: integer sample weights (0 = not in the tree); tree_state[n_trees]: the splitter's
        generator state; tree_fit[n_trees]: the fit a tree belongs to; per fit the criterion (0 / 'gini', 1 / 'entropy'),
        max_depth (0 / None = no limit), max_features (a number of columns), min_samples_leaf, min_samples_split;
        export[n_trees]: which trees' node arrays to return (None: all).  Returns (sum0[n_fits][n], sum1[n_fits][n], trees):
        the two class fractions of every sample's leaves added in tree order, and per tree None or a dict of node_count,
        max_depth, feature / left / right / n_node_samples / counts[:, 2] (weighted) / impurity by node (pre-order), leaf[n]."""
        return self._forest_fit(False, np.ascontiguousarray(X, dtype=np.float32), y01, tree_weight, tree_state, tree_fit, fit_criterion,
                                fit_max_depth, fit_max_features, fit_min_samples_leaf, fit_min_samples_split, export)

    def forest_fit_counts(self, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                          fit_min_samples_leaf, fit_min_samples_split, export=None):
        """forest_fit on a count design (psk_forest_fit_counts): integers in 0 .. 2^24, ValueError otherwise.  The same
        results, every tree's dict with threshold by node as tree_fit_counts returns it."""
        return self._forest_fit(True, self._count_design(X, "forest_fit_counts"), y01, tree_weight, tree_state, tree_fit, fit_criterion,
                                fit_max_depth, fit_max_features, fit_min_samples_leaf, fit_min_samples_split, export)

    def forest_fit_real(self, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                        fit_min_samples_leaf, fit_min_samples_split, export=None):
        """forest_fit_counts on a design of any finite float32 values (psk_forest_fit_real), ValueError on a NaN or an
        infinity.  The same results; equal values as tree_fit_real takes them."""
        return self._forest_fit("real", self._real_design(X, "forest_fit_real"), y01, tree_weight, tree_state, tree_fit, fit_criterion,
                                fit_max_depth, fit_max_features, fit_min_samples_leaf, fit_min_samples_split, export)

    def _forest_fit(self, counts, X, y01, tree_weight, tree_state, tree_fit, fit_criterion, fit_max_depth, fit_max_features,
                    fit_min_samples_leaf, fit_min_samples_split, export):
        n, p = X.shape
        y = np.ascontiguousarray(y01, dtype=np.int32)
        wt = np.asarray(tree_weight)
        if wt.ndim != 2 or wt.shape[1] != n or wt.min() < 0 or wt.max() > 65535:
            raise ValueError("tree_weight must be [n_trees][n] integers in 0..65535")
        wt = np.ascontiguousarray(wt, dtype=np.uint16)
        nt = wt.shape[0]
        state = np.ascontiguousarray(tree_state, dtype=np.uint32)
        tfit = np.ascontiguousarray(tree_fit, dtype=np.int32)
        flag = np.ones(nt, dtype=np.int32) if export is None else np.ascontiguousarray(np.asarray(export) != 0, dtype=np.int32)
        crit = np.ascontiguousarray([{"gini": 0, "entropy": 1}.get(c, c) for c in fit_criterion], dtype=np.int32)
        depth = np.ascontiguousarray([d or 0 for d in fit_max_depth], dtype=np.int32)
        mf = np.ascontiguousarray(fit_max_features, dtype=np.int32)
        msl = np.ascontiguousarray(fit_min_samples_leaf, dtype=np.int32)
        mss = np.ascontiguousarray(fit_min_samples_split, dtype=np.int32)
        nf = len(crit)
        if not (len(state) == len(tfit) == len(flag) == nt and len(depth) == len(mf) == len(msl) == len(mss) == nf):
            raise ValueError("per-tree arrays must have n_trees entries and per-fit arrays n_fits")
        n_exp = int(flag.sum())
        pool = int((2 * (wt[flag != 0] != 0).sum(axis=1) - 1).sum()) if n_exp else 0
        sum0, sum1 = np.zeros((nf, n)), np.zeros((nf, n))
        count, deepest, off = np.zeros(nt, dtype=np.int32), np.zeros(nt, dtype=np.int32), np.zeros(nt, dtype=np.int64)
        nodes, imp, leaf = np.zeros((max(pool, 1), 6), dtype=np.int32), np.zeros(max(pool, 1)), np.zeros((max(n_exp, 1), n), dtype=np.int32)
        args = (self._h, _ptr(X), _ptr(y), n, p, nt, _ptr(wt), _ptr(state), _ptr(tfit), _ptr(flag), nf, _ptr(crit), _ptr(depth), _ptr(mf),
                _ptr(msl), _ptr(mss), _ptr(sum0), _ptr(sum1), _ptr(count), _ptr(deepest), pool, _ptr(off), _ptr(nodes), _ptr(imp), _ptr(leaf))
        thr = np.zeros(max(pool, 1)) if counts else None
        if counts:
            name = "psk_forest_fit_real" if counts == "real" else "psk_forest_fit_counts"
            self._check(getattr(self._lib, name)(*args, _ptr(thr)), name)
        else:
            self._check(self._lib.psk_forest_fit(*args), "psk_forest_fit")
        trees, row = [], 0
        for t in range(nt):
            if not flag[t]:
                trees.append(None)
                continue
            a, k = int(off[t]), int(count[t])
            trees.append(self._tree_dict(nodes[a:a + k], imp[a:a + k], deepest[t], leaf[row], thr[a:a + k] if counts else None))
            row += 1
        return sum0, sum1, trees

    def nb_fit(self, X, y01, fold, fit_fold):
        """Bernoulli naive-Bayes counts (psk_nb_fit) on a 0/1 design, every fit in one call; fit_fold[j] = -1: all samples.
        Returns (feature_count[n_fits][2][p], class_count[n_fits][2]), int32: per class the training samples that carry
        each k-mer, and the training samples."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        n, p = X.shape
        y = np.ascontiguousarray(y01, dtype=np.int32)
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        fit_fold = np.ascontiguousarray(fit_fold, dtype=np.int32)
        if len(y) != n or len(fold) != n or fit_fold.ndim != 1:
            raise ValueError("y01 and fold must have one entry per row of X, fit_fold one per fit")
        nf = len(fit_fold)
        fc, cc = np.zeros((nf, 2, p), dtype=np.int32), np.zeros((nf, 2), dtype=np.int32)
        self._check(self._lib.psk_nb_fit(self._h, _ptr(X), _ptr(y), n, p, _ptr(fold), _ptr(fit_fold), nf, _ptr(fc), _ptr(cc)), "psk_nb_fit")
        return fc, cc

    def nb_jll(self, X, delta, class_log_prior, neg_sum):
        """Joint log-likelihoods of the rows of a 0/1 design under Bernoulli naive-Bayes models (psk_nb_jll):
        delta[n_models][2][p] = feature_log_prob_ - log(1 - exp(feature_log_prob_)), class_log_prior[n_models][2],
        neg_sum[n_models][2] (one model: the leading axis may be left out).  Returns jll[n_models][n][2] (one model:
        jll[n][2]) in the summation order include/psk.h states."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        n, p = X.shape
        delta = np.ascontiguousarray(delta, dtype=np.float64)
        one = delta.ndim == 2
        delta = delta.reshape(-1, 2, p)
        nm = delta.shape[0]
        prior = np.ascontiguousarray(class_log_prior, dtype=np.float64).reshape(nm, 2)
        neg = np.ascontiguousarray(neg_sum, dtype=np.float64).reshape(nm, 2)
        jll = np.zeros((nm, n, 2))
        self._check(self._lib.psk_nb_jll(self._h, _ptr(X), n, p, _ptr(delta), nm, _ptr(prior), _ptr(neg), _ptr(jll)), "psk_nb_jll")
        return jll[0] if one else jll

    GB_LOSSES = {"squared_error": 0, "log_loss": 1}

    def gb_fit(self, X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, staged=True):
        """Gradient-boosted regression trees (psk_gb_fit: scikit-learn's gradient boosting, include/psk.h f16) on a 0/1 design,
        every fit in one call; fit_fold[j] = -1: all samples in bag.  loss: 0 / 'squared_error' or 1 / 'log_loss' (y 0/1);
        init_raw[n_fits]: the raw prediction before stage 0.  Returns one dictionary per fit: node_count[n_estimators],
        nodes[n_estimators][cap][4] (feature, -2 at a leaf; left; right, -1 at a leaf; in-bag n_node_samples), value and
        impurity[n_estimators][cap], cap = 2^(max_depth + 1) - 1, raw[n] (every sample's raw prediction after the last stage)
        and staged[n_estimators][n] (after each stage; None unless asked for)."""
        return self._gb_fit(False, np.ascontiguousarray(X, dtype=np.float32), y, fold, fit_fold, loss, n_estimators, learning_rate,
                            max_depth, init_raw, staged)

    def gb_fit_counts(self, X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, staged=True):
        """gb_fit on a count design (psk_gb_fit_counts): integers in 0 .. 2^24, ValueError otherwise.  The same dictionaries,
        nodes[..][0] the design column of a split, plus threshold[n_estimators][cap]: scikit-learn's midpoint between the two
        values around the split among the node's in-bag samples, -2 at a leaf and behind node_count; x <= threshold goes left."""
        return self._gb_fit(True, self._count_design(X, "gb_fit_counts"), y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth,
                            init_raw, staged)

    def _gb_fit(self, counts, X, y, fold, fit_fold, loss, n_estimators, learning_rate, max_depth, init_raw, staged):
        n, p = X.shape
        y = np.ascontiguousarray(y, dtype=np.float64)
        fold = np.ascontiguousarray(fold, dtype=np.int32)
        fit_fold = np.ascontiguousarray(fit_fold, dtype=np.int32)
        init = np.ascontiguousarray(init_raw, dtype=np.float64).reshape(-1)
        if len(y) != n or len(fold) != n or fit_fold.ndim != 1 or len(init) != len(fit_fold):
            raise ValueError("y and fold must have one entry per row of X, fit_fold and init_raw one per fit")
        nf, ne, depth = len(fit_fold), int(n_estimators), int(max_depth)
        # (the library refuses these too; the output arrays are sized by them, so they are clamped for the allocation only)
        cap = (2 << min(max(depth, 1), 10)) - 1
        rows = min(max(ne, 1), 1000)
        count = np.zeros((nf, rows), dtype=np.int32)
        nodes = np.zeros((nf, rows, cap, 4), dtype=np.int32)
        value, imp = np.zeros((nf, rows, cap)), np.zeros((nf, rows, cap))
        raw = np.zeros((nf, n))
        stg = np.zeros((nf, rows, n)) if staged else None
        head = (self._h, _ptr(X), _ptr(y), n, p, _ptr(fold), _ptr(fit_fold), nf, int(self.GB_LOSSES.get(loss, loss)), ne, float(learning_rate),
                depth, _ptr(init), _ptr(count), _ptr(nodes), _ptr(value), _ptr(imp))
        if not counts:
            self._check(self._lib.psk_gb_fit(*head, _ptr(raw), _ptr(stg)), "psk_gb_fit")
        else:
            thr = np.zeros((nf, rows, cap))
            self._check(self._lib.psk_gb_fit_counts(*head, _ptr(thr), _ptr(raw), _ptr(stg)), "psk_gb_fit_counts")
        fits = [dict(node_count=count[j], nodes=nodes[j], value=value[j], impurity=imp[j], raw=raw[j], staged=stg[j] if staged else None)
                for j in range(nf)]
        if counts:
            for j in range(nf):
                fits[j]["threshold"] = thr[j]
        return fits

    def gb_decision(self, X, node_count, nodes, value, init_raw, learning_rate, max_depth):
        """The raw predictions of the rows of a 0/1 design under one gradient-boosting model in gb_fit's layout
        (psk_gb_decision): init_raw, then + learning_rate * value[leaf] stage after stage.  Returns raw[n]."""
        return self._gb_decision(np.ascontiguousarray(X, dtype=np.float32), node_count, nodes, value, None, init_raw, learning_rate, max_depth)

    def gb_decision_counts(self, X, node_count, nodes, value, threshold, init_raw, learning_rate, max_depth):
        """gb_decision for a model of gb_fit_counts on the rows of a count design (psk_gb_decision_counts): x <= threshold goes
        left.  threshold[n_estimators][cap] beside nodes and value.  Returns raw[n]."""
        return self._gb_decision(self._count_design(X, "gb_decision_counts"), node_count, nodes, value, threshold, init_raw, learning_rate,
                                 max_depth)

    def _gb_decision(self, X, node_count, nodes, value, threshold, init_raw, learning_rate, max_depth):
        n, p = X.shape
        depth = int(max_depth)
        cap = (2 << min(max(depth, 1), 10)) - 1
        count = np.ascontiguousarray(node_count, dtype=np.int32).reshape(-1)
        ne = len(count)
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        value = np.ascontiguousarray(value, dtype=np.float64)
        if nodes.shape != (ne, cap, 4) or value.shape != (ne, cap):
            raise ValueError("nodes must be [n_estimators][%d][4] and value [n_estimators][%d] for max_depth %d" % (cap, cap, depth))
        raw = np.zeros(n)
        if threshold is None:
            self._check(self._lib.psk_gb_decision(self._h, _ptr(X), n, p, ne, depth, _ptr(count), _ptr(nodes), _ptr(value), float(init_raw),
                                                  float(learning_rate), _ptr(raw)), "psk_gb_decision")
            return raw
        thr = np.ascontiguousarray(threshold, dtype=np.float64)
        if thr.shape != (ne, cap):
            raise ValueError("threshold must be [n_estimators][%d] for max_depth %d" % (cap, depth))
        self._check(self._lib.psk_gb_decision_counts(self._h, _ptr(X), n, p, ne, depth, _ptr(count), _ptr(nodes), _ptr(value), _ptr(thr),
                                                     float(init_raw), float(learning_rate), _ptr(raw)), "psk_gb_decision_counts")
        return raw

    def pca_fit(self, X, n_comp=None):
        """StandardScaler + PCA of a design (psk_pca_fit): X[n][p], presence or counts; n_comp leading components, all
        min(n, p) when None.  Returns a dictionary: mean[p], var[p], scale[p], lambda[min(n, p)] (eigenvalues of Z Z',
        descending), scores[n][n_comp], components[n_comp][p] and sweeps (of the eigen-solver)."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("X must be samples x columns")
        n, p = X.shape
        k = min(n, p) if n_comp is None else int(n_comp)
        mean, var, scale = np.zeros(p), np.zeros(p), np.zeros(p)
        lam, scores, comp = np.zeros(min(n, p)), np.zeros((n, max(k, 0))), np.zeros((max(k, 0), p))
        sweeps = ctypes.c_int32()
        self._check(self._lib.psk_pca_fit(self._h, _ptr(X), n, p, k, _ptr(mean), _ptr(var), _ptr(scale), _ptr(lam), _ptr(scores),
                                          _ptr(comp), ctypes.addressof(sweeps)), "psk_pca_fit")
        return {"mean": mean, "var": var, "scale": scale, "lambda": lam, "scores": scores, "components": comp, "sweeps": int(sweeps.value)}

    def pca_transform(self, X, center, scale, components):
        """scores[m][k] = ((X - center) / scale) . components' (psk_pca_transform) in the summation order include/psk.h states:
        a row's scores depend on that row and the model only."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2:
            raise ValueError("X must be samples x columns")
        m, p = X.shape
        center = np.ascontiguousarray(center, dtype=np.float64)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        comp = np.ascontiguousarray(components, dtype=np.float64)
        if center.shape != (p,) or scale.shape != (p,) or comp.ndim != 2 or comp.shape[1] != p:
            raise ValueError("center and scale must have one entry per column of X, components one row of them per component")
        k = comp.shape[0]
        scores = np.zeros((m, k))
        self._check(self._lib.psk_pca_transform(self._h, _ptr(X), m, p, _ptr(center), _ptr(scale), _ptr(comp), k, _ptr(scores)),
                    "psk_pca_transform")
        return scores

    # -- k-mer assembly ---------------------------------------------------------------------------------
    def asm_round(self, strings, min_olap, pair_cap=None):
        """One round's matching of the assembly (psk_asm_round) over a list of ACGT strings: returns (pairs[n_pairs][3] int32 --
        (a, b, t) per ordered pair of different list positions, t the largest overlap of at least min_olap bases, in no
        particular order --, contained[n] bool: the string lies inside a different string).  pair_cap: room for that many
        pairs, n (n - 1) when None.  More pairs than that: PskError with code PSK_ERANGE, whose n_pairs is the true number."""
        n = len(strings)
        words, word_off, lens = pack_strings(strings)
        cap = n * (n - 1) if pair_cap is None else int(pair_cap)
        pairs = np.zeros((max(cap, 1), 3), dtype=np.int32)
        contained = np.zeros(max(n, 1), dtype=np.uint8)
        n_pairs = ctypes.c_uint64()
        rc = self._lib.psk_asm_round(self._h, _ptr(words), _ptr(word_off), _ptr(lens), n, int(min_olap), cap, _ptr(pairs), ctypes.byref(n_pairs),
                                     _ptr(contained))
        try:
            self._check(rc, "psk_asm_round")
        except PskError as e:
            e.n_pairs = int(n_pairs.value)
            raise
        return pairs[:int(n_pairs.value)].copy(), contained[:n].astype(bool)

    def assemble(self, kmer_words, k, both_strands=False):
        """The assembly of k-mers given as 2k-bit words (psk_assemble; formats.kmer_to_word): returns (sequences in the output's
        order -- longest first, lexicographically among equal lengths --, rounds that merged something).  A cap of the loop
        (PSK_ASM_MAX_STRINGS, PSK_ASM_MAX_PAIRS, PSK_ASM_MAX_LEN) raises PskError with code PSK_ERANGE."""
        words = np.ascontiguousarray(kmer_words, dtype=np.uint64)
        n = len(words)
        cap = max(1 << 16, 8 * n * (int(k) + 1))
        for _ in range(2):
            text = ctypes.create_string_buffer(cap)
            n_seqs, text_len, rounds = ctypes.c_int64(), ctypes.c_uint64(), ctypes.c_int32()
            rc = self._lib.psk_assemble(self._h, _ptr(words), n, int(k), 1 if both_strands else 0, text, cap, ctypes.byref(n_seqs),
                                        ctypes.byref(text_len), ctypes.byref(rounds))
            if rc == _lib.PSK_ERANGE and text_len.value > cap:     # the text did not fit: once more with the room it asked for
                cap = int(text_len.value)
                continue
            break
        self._check(rc, "psk_assemble")
        seqs = text.raw[:text_len.value].decode("ascii").split("\n") if n_seqs.value else []
        return seqs, int(rounds.value)

    # -- population-structure weights --------------------------------------------------------------
    def minhash_sketch(self, data, k=21, sketch_size=1000, seed=42):
        data = bytes(data)
        out = np.zeros(int(sketch_size), dtype=np.uint64)
        n = ctypes.c_uint64()
        self._check(self._lib.psk_minhash_sketch(self._h, data, len(data), int(k), int(sketch_size), int(seed),
                                                 _ptr(out), ctypes.byref(n)), "psk_minhash_sketch")
        return out[: n.value].copy()

    def mash_pairs(self, sketches, sketch_size=1000):
        """sketches: list of ascending hash lists.  Returns (common[n][n], denom[n][n]) of Mash's Jaccard estimate."""
        n = len(sketches)
        sk = np.zeros((n, int(sketch_size)), dtype=np.uint64)
        lens = np.zeros(n, dtype=np.uint32)
        for i, h in enumerate(sketches):
            h = np.asarray(h, dtype=np.uint64)[: int(sketch_size)]
            sk[i, : len(h)] = h
            lens[i] = len(h)
        common = np.zeros((n, n), dtype=np.uint32)
        denom = np.zeros((n, n), dtype=np.uint32)
        self._check(self._lib.psk_mash_pairs(self._h, _ptr(sk), _ptr(lens), n, int(sketch_size), _ptr(common), _ptr(denom)),
                    "psk_mash_pairs")
        return common, denom

    def nj_merges(self, dist):
        """Neighbour-joining merge list of a symmetric distance matrix (psk_nj_merges)."""
        d = np.ascontiguousarray(dist, dtype=np.float64)
        n = d.shape[0]
        mi = np.zeros(n - 2, dtype=np.int32)
        mj = np.zeros(n - 2, dtype=np.int32)
        d1 = np.zeros(n - 2)
        d2 = np.zeros(n - 2)
        last = np.zeros(1)
        self._check(self._lib.psk_nj_merges(self._h, _ptr(d), n, _ptr(mi), _ptr(mj), _ptr(d1), _ptr(d2), _ptr(last)),
                    "psk_nj_merges")
        return mi, mj, d1, d2, float(last[0])

    # -- prediction -------------------------------------------------------------------------------
    def count_dict(self, data, k, dict_words):
        data = bytes(data)
        d = np.ascontiguousarray(dict_words, dtype=np.uint64)
        out = np.zeros(len(d), dtype=np.uint32)
        self._check(self._lib.psk_count_dict(self._h, data, len(data), int(k), _ptr(d), len(d), _ptr(out)),
                    "psk_count_dict")
        return out


    def count_dict_batch(self, datas, k, dict_words, n_threads=4):
        """psk_count_dict_batch: every sample (file image) against one dictionary -> counts[n][n_dict]."""
        datas = [bytes(d) for d in datas]
        n = len(datas)
        d = np.ascontiguousarray(dict_words, dtype=np.uint64)
        out = np.zeros((n, len(d)), dtype=np.uint32)
        if n and len(d):
            arr = (ctypes.c_char_p * n)(*datas)
            lens = (ctypes.c_size_t * n)(*[len(x) for x in datas])
            self._check(self._lib.psk_count_dict_batch(self._h, n, arr, lens, int(k), _ptr(d), len(d), _ptr(out), int(n_threads)),
                        "psk_count_dict_batch")
        return out

    def count_dict_files(self, paths, k, dict_words, n_threads=4):
        """psk_count_dict_files: the same for UNCOMPRESSED files, read by the library's framing threads."""
        enc = [os.fsencode(p) for p in paths]
        n = len(enc)
        d = np.ascontiguousarray(dict_words, dtype=np.uint64)
        out = np.zeros((n, len(d)), dtype=np.uint32)
        if n and len(d):
            arr = (ctypes.c_char_p * n)(*enc)
            sizes = (ctypes.c_size_t * n)(*[os.path.getsize(p) for p in paths])
            self._check(self._lib.psk_count_dict_files(self._h, n, arr, sizes, int(k), _ptr(d), len(d), _ptr(out), int(n_threads)),
                        "psk_count_dict_files")
        return out


    def frame_sequence_gpu(self, data):
        """psk_frame_sequence_gpu: the clean stream as the device framing produces it (r06: FASTQ that is not four lines per
        record included -- the scan of line kinds of frame_gpu.hip; until r05 such input came back as None: the host's)."""
        data = bytes(data)
        out = np.empty(len(data) + 128, dtype=np.uint8)
        n = self._lib.psk_frame_sequence_gpu(self._h, data, len(data), _ptr(out), out.size)
        if n == -5:
            return None
        if n < 0:
            self._check(int(n), "psk_frame_sequence_gpu")
        return out[:n].tobytes()


def frame_sequence(data):
    """Host-only tokeniser framing (psk_frame_sequence): the clean stream handed to the GPU."""
    lib = _lib.load()
    data = bytes(data)
    out = np.zeros(max(len(data), 1), dtype=np.uint8)
    n = lib.psk_frame_sequence(data, len(data), out.ctypes.data, len(out))
    if n < 0:
        raise PskError("psk_frame_sequence failed: %d" % n)
    return out[:n].tobytes()


SCAN_FORMS = ("dense", "cx", "cx_side", "cx_side_pc", "cx_side_idx")     # Chi2Form, csrc/chi2_plan.h


def cx_idx_plan(feas, pc_hist, n_ov, knob_on=True):
    """(ranges [(begin, len)] kept (at most 4), all ranges there are, rows in them, the index form is chosen) for the
    feasible popcounts `feas` (a set) and the histogram pc_hist: psk_cx_idx_plan (host code, no device)."""
    lib = _lib.load()
    fw = (ctypes.c_uint64 * 4)()
    for pc in feas:
        fw[pc >> 6] |= 1 << (pc & 63)
    hist = (ctypes.c_uint64 * max(len(pc_hist), 1))(*[int(h) for h in pc_hist])
    begin, length = (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 4)()
    n_runs, rows, chosen = ctypes.c_int(), ctypes.c_uint64(), ctypes.c_int()
    rc = lib.psk_cx_idx_plan(fw, hist, len(pc_hist), int(n_ov), int(bool(knob_on)), begin, length, ctypes.byref(n_runs),
                             ctypes.byref(rows), ctypes.byref(chosen))
    if rc < 0:
        raise PskError("psk_cx_idx_plan failed: %d" % rc)
    return [(begin[i], length[i]) for i in range(min(n_runs.value, 4))], n_runs.value, rows.value, bool(chosen.value)


def cx_idx_shape(n_rows, cap_blocks):
    """(workgroups, rows per workgroup, threads per workgroup, entries per result segment) of the index form for n_rows
    feasible rows: psk_cx_idx_shape (host code, no device)."""
    lib = _lib.load()
    blocks, rpb, thr, cap = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint64()
    rc = lib.psk_cx_idx_shape(int(n_rows), int(cap_blocks), ctypes.byref(blocks), ctypes.byref(rpb), ctypes.byref(thr), ctypes.byref(cap))
    if rc < 0:
        raise PskError("psk_cx_idx_shape failed: %d" % rc)
    return blocks.value, rpb.value, thr.value, cap.value


def cx_pc_plan(n1, n0, n_samples, min_samples, max_samples, thr):
    """The popcounts (a set of ints below 256) a side-matrix row may have for a chi2 scan with these parameters to keep
    it (psk_cx_pc_plan: host code, no device)."""
    lib = _lib.load()
    feas = (ctypes.c_uint64 * 4)()
    rc = lib.psk_cx_pc_plan(n1, n0, n_samples, min_samples, max_samples, thr, feas)
    if rc < 0:
        raise PskError("psk_cx_pc_plan failed: %d" % rc)
    return {pc for pc in range(256) if (feas[pc >> 6] >> (pc & 63)) & 1}
