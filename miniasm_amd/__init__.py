"""miniasm_amd -- MI355X-native overlap-graph hot path of miniasm (PAF hits -> string graph -> GFA).

The product is native: hand-written HIP kernels (miniasm_amd/csrc) behind a C ABI (include/mahip.h), host C
that mirrors the reference's link interface (include/miniasm_amd.h, miniasm_amd/host) and the `miniasm`
command line (miniasm_amd/bin/miniasm).  This Python module is only the thin ctypes harness that tests and
bench.py use to drive the C ABI; it contains no compute and no fallback path: without the built library, or
without a GPU, calls fail loudly.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "miniasm_amd")
LIB_PATH = os.environ.get("MINIASM_AMD_LIB") or os.path.join(PKG, "lib", "libminiasm_amd.so")  # the override is for kernel-variant experiments (tools/variants.sh)
CLI_PATH = os.path.join(PKG, "bin", "miniasm")
PAFGEN_PATH = os.path.join(PKG, "bin", "pafgen")

# byte layouts of the reference records (miniasm.h:29-40, asg.h:7-15), as numpy structured dtypes
HIT_DT = np.dtype([("qns", "<u8"), ("qe", "<u4"), ("tn", "<u4"), ("ts", "<u4"), ("te", "<u4"), ("mlrev", "<u4"), ("bldel", "<u4")])
SUB_DT = np.dtype([("sdel", "<u4"), ("e", "<u4")])
ARC_DT = np.dtype([("ul", "<u8"), ("v", "<u4"), ("oldel", "<u4")])
assert HIT_DT.itemsize == 32 and SUB_DT.itemsize == 8 and ARC_DT.itemsize == 16


SHARD_N_PHASES = 16
SHARD_PHASE_NAMES = ["sort", "sub#1", "x:sub0", "cut+flt+sub#2", "x:sub1", "merge+cut+contained", "x:flags", "squeeze+sg flags", "x:seq.del", "local arcs",
                     "x:arc counts", "x:arc blocks", "tie repair", "reduction (own vertices)", "x:del flags", "rank 0: cleanup+symm"]  # host/sharded.c: ma_shard_phase_name


class ShardStats(C.Structure):  # host/ma_host.h: ma_shard_stats_t
    _fields_ = [("n_rem1", C.c_uint64), ("n_rem2", C.c_uint64), ("n_hits", C.c_uint64), ("n_seq_new", C.c_uint32), ("n_arc", C.c_uint32), ("n_loc_arc", C.c_uint32),
                ("n_red", C.c_uint32), ("n_multi", C.c_uint32), ("n_asymm", C.c_uint32), ("tie_groups", C.c_uint64), ("push_conflicts", C.c_uint64), ("tie_repaired", C.c_int),
                ("n_red_local", C.c_uint32), ("reduced", C.c_int), ("have_phases", C.c_int), ("phase_ms", C.c_float * SHARD_N_PHASES), ("xchg_bytes", C.c_uint64 * SHARD_N_PHASES)]


class MaOpt(C.Structure):  # miniasm.h:12-27
    _fields_ = [("min_span", C.c_int), ("min_match", C.c_int), ("min_dp", C.c_int), ("min_iden", C.c_float),
                ("max_hang", C.c_int), ("min_ovlp", C.c_int), ("int_frac", C.c_float),
                ("gap_fuzz", C.c_int), ("n_rounds", C.c_int), ("bub_dist", C.c_int), ("max_ext", C.c_int),
                ("min_ovlp_drop_ratio", C.c_float), ("max_ovlp_drop_ratio", C.c_float), ("final_ovlp_drop_ratio", C.c_float)]


class SdSeq(C.Structure):  # sdict.h:6-9
    _fields_ = [("name", C.c_char_p), ("len", C.c_uint32), ("auxdel", C.c_uint32)]


class Sdict(C.Structure):  # sdict.h:11-15
    _fields_ = [("n_seq", C.c_uint32), ("m_seq", C.c_uint32), ("seq", C.POINTER(SdSeq)), ("h", C.c_void_p)]


class Asg(C.Structure):  # asg.h:17-23
    _fields_ = [("m_arc", C.c_uint32), ("n_arc_srt", C.c_uint32), ("arc", C.c_void_p),
                ("m_seq", C.c_uint32), ("n_seq_symm", C.c_uint32), ("seq", C.c_void_p), ("idx", C.c_void_p)]

    @property
    def n_arc(self):
        return self.n_arc_srt & 0x7FFFFFFF

    @property
    def n_seq(self):
        return self.n_seq_symm & 0x7FFFFFFF


class TieInfo(C.Structure):  # include/mahip.h: mahip_tie_info_t
    _fields_ = [("arc_tie_groups", C.c_uint64), ("arc_tie_arcs", C.c_uint64), ("push_conflicts", C.c_uint64), ("hit_ties", C.c_uint64),
                ("arc_walk", C.c_int), ("hit_walk", C.c_int), ("unrepaired", C.c_int), ("push_conflicts_seen", C.c_uint64), ("hit_walk_reads", C.c_uint64)]


class FastxInfo(C.Structure):  # include/mahip.h: mahip_fastx_info_t
    _fields_ = [("format", C.c_int), ("n_lines", C.c_uint64), ("n_records", C.c_uint64), ("n_cr", C.c_uint64), ("regular", C.c_int), ("reason", C.c_int)]


class UseqWant(C.Structure):  # include/mahip.h: mahip_useq_want_t
    _fields_ = [("dst_off", C.c_uint64), ("name_off", C.c_uint64), ("name_len", C.c_uint32), ("len", C.c_uint32), ("s", C.c_uint32), ("e", C.c_uint32),
                ("rev", C.c_uint32), ("whole", C.c_uint32)]


class UseqInfo(C.Structure):  # include/mahip.h: mahip_useq_info_t
    _fields_ = [("reader", C.c_int), ("reason", C.c_int), ("format", C.c_int), ("n_records", C.c_uint64), ("n_matched", C.c_uint64), ("n_dup", C.c_uint64),
                ("n_short", C.c_uint64)]


class UseqPlanInfo(C.Structure):  # include/mahip.h: mahip_useq_plan_info_t
    _fields_ = [("road", C.c_int), ("reason", C.c_int), ("n_utg", C.c_uint64), ("n_members", C.c_uint64), ("n_reads", C.c_uint64), ("n_wanted", C.c_uint64), ("name_bytes", C.c_uint64),
                ("blob_bytes", C.c_uint64), ("arena_bytes", C.c_uint64), ("n_multi", C.c_uint64), ("uoff_tiles", C.c_uint64), ("ms", C.c_double)]


PLAN_ROADS = {0: None, 1: "host", 2: "device"}
PLAN_REASONS = ["OK", "NO_UG", "NO_NAMES", "MULTI", "NOMEM", "FORCED"]
WANT_DT = np.dtype([("dst_off", "<u8"), ("name_off", "<u8"), ("name_len", "<u4"), ("len", "<u4"), ("s", "<u4"), ("e", "<u4"), ("rev", "<u4"), ("whole", "<u4")])  # mahip_useq_want_t
PLACE_DT = np.dtype([("utg", "<u4"), ("start", "<u4"), ("len", "<u4"), ("ori", "<u4")])  # mahip_useq_place_t


def _plan_dict(p):
    d = {k: getattr(p, k) for k, _ in UseqPlanInfo._fields_}
    d.update(road=PLAN_ROADS.get(p.road), reason=PLAN_REASONS[p.reason])
    return d


class UseqStreamVerdict(C.Structure):  # include/mahip.h: mahip_useq_stream_verdict_t
    _fields_ = [("reason", C.c_int), ("n_records", C.c_uint64), ("bytes_consumed", C.c_uint64), ("carry_bytes", C.c_uint64), ("n_placed", C.c_uint64)]


class UseqStreamReport(C.Structure):  # include/mahip.h: mahip_useq_stream_report_t
    _fields_ = [("format", C.c_int), ("n_pieces", C.c_uint64), ("n_records", C.c_uint64), ("n_matched", C.c_uint64), ("n_dup", C.c_uint64), ("n_short", C.c_uint64),
                ("n_jobs", C.c_uint64), ("max_carry", C.c_uint64), ("n_window_grow", C.c_uint32), ("refused_reason", C.c_int), ("refused_piece", C.c_int64),
                ("laps_ms", C.c_double * 4)]


# include/mahip.h: MAHIP_FASTX_* reasons, formats, MAHIP_USEQ_* readers
FASTX_REASONS = ["OK", "CR", "FIRST_BYTE", "FASTA_LINE_START", "FASTQ_SHAPE", "FASTQ_QUAL_LEN", "TOO_MANY_LINES", "NOMEM", "SHORT_READ", "NOT_PLAIN", "FORCED", "NUL_BYTE", "LONG_LINE"]
FASTX_FORMATS = {0: None, 1: "fasta", 2: "fastq"}
USEQ_READERS = {0: None, 1: "host", 2: "device", 3: "stream"}


class BgzfInfo(C.Structure):  # include/mahip.h: mahip_bgzf_info_t
    _fields_ = [("n_members", C.c_uint64), ("n_empty", C.c_uint64), ("n_stored", C.c_uint64), ("n_fixed", C.c_uint64), ("n_dynamic", C.c_uint64),
                ("comp_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("reader", C.c_int), ("reason", C.c_int), ("first_bad_member", C.c_int64),
                ("laps_ms", C.c_double * 4)]


# include/mahip.h: MAHIP_BGZF_* reasons, readers, targets
BGZF_REASONS = ["OK", "NOT_BGZF", "NO_BC", "PAST_END", "TRAILING", "BAD_FLG", "ISIZE", "BAD_BTYPE", "STORED_LEN", "BAD_LENGTHS", "BAD_SYMBOL", "DIST_TOO_FAR", "OUT_OVERFLOW",
                "IN_EXHAUSTED", "OUT_SHORT", "CRC", "NOMEM", "NOT_SEEKABLE", "FORCED", "EMPTY"]
BGZF_READERS = {0: None, 1: "host", 2: "device"}
BGZF_TARGETS = {"paf": 1, "fastx": 2}


def _bgzf_dict(b):
    return dict(n_members=b.n_members, n_empty=b.n_empty, n_stored=b.n_stored, n_fixed=b.n_fixed, n_dynamic=b.n_dynamic, comp_bytes=b.comp_bytes, text_bytes=b.text_bytes,
                reader=BGZF_READERS[b.reader], reason=BGZF_REASONS[b.reason], first_bad_member=b.first_bad_member, laps_ms=dict(zip(("walk", "upload", "inflate", "crc"), b.laps_ms)))


class BgzfRange(C.Structure):  # include/mahip.h: mahip_bgzf_range_t
    _fields_ = [("text_bytes", C.c_uint64), ("beg", C.c_uint64), ("end", C.c_uint64), ("first_member", C.c_uint64), ("n_members_inflated", C.c_uint64),
                ("comp_bytes_uploaded", C.c_uint64), ("n_rounds", C.c_int)]


BGZF_RANGE_AHEAD = 1  # include/mahip.h: MAHIP_BGZF_RANGE_AHEAD


def _bgzf_range_dict(r):
    return dict(text_bytes=r.text_bytes, beg=r.beg, end=r.end, first_member=r.first_member, n_members_inflated=r.n_members_inflated, comp_bytes_uploaded=r.comp_bytes_uploaded,
                n_rounds=r.n_rounds)


class GzipInfo(C.Structure):  # include/mahip.h: mahip_gzip_info_t
    _fields_ = [("comp_bytes", C.c_uint64), ("text_bytes", C.c_uint64), ("chunk", C.c_uint64), ("n_chunks", C.c_uint64), ("n_synced", C.c_uint64), ("n_items", C.c_uint64),
                ("n_stored", C.c_uint64), ("n_fixed", C.c_uint64), ("n_dynamic", C.c_uint64), ("reader", C.c_int), ("reason", C.c_int), ("first_bad_item", C.c_int64),
                ("laps_ms", C.c_double * 6)]


class GzipItem(C.Structure):  # include/mahip.h: mahip_gzip_item_t
    _fields_ = [("sync_bit", C.c_int64), ("end_bit", C.c_uint64), ("out_len", C.c_uint64), ("status", C.c_uint32), ("flags", C.c_uint32)]


# include/mahip.h: MAHIP_GZIP_* reasons
GZIP_REASONS = ["OK", "BAD_HEADER", "MULTI_MEMBER", "NO_SYNC", "SYNC_MISMATCH", "ISIZE", "BAD_BTYPE", "STORED_LEN", "BAD_LENGTHS", "BAD_SYMBOL", "DIST_TOO_FAR", "OUT_OVERFLOW",
                "IN_EXHAUSTED", "OUT_SHORT", "CRC", "NOMEM", "NOT_SEEKABLE", "FORCED", "EMPTY", "TOO_MANY_CANDIDATES"]


class GzipMembersInfo(C.Structure):  # include/mahip.h: mahip_gzip_members_info_t
    _fields_ = [("n_members", C.c_uint64), ("n_candidates", C.c_uint64), ("n_heads", C.c_uint64), ("bad_member", C.c_int64), ("cand_cap", C.c_uint64), ("laps_ms", C.c_double * 2)]


class GzipMember(C.Structure):  # include/mahip.h: mahip_gzip_member_t
    _fields_ = [("comp_off", C.c_uint64), ("hdr_len", C.c_uint64), ("text_off", C.c_uint64), ("text_len", C.c_uint64), ("crc", C.c_uint32), ("isize", C.c_uint32), ("n_items", C.c_uint64)]


def _gzip_dict(g):
    return dict(comp_bytes=g.comp_bytes, text_bytes=g.text_bytes, chunk=g.chunk, n_chunks=g.n_chunks, n_synced=g.n_synced, n_items=g.n_items, n_stored=g.n_stored, n_fixed=g.n_fixed,
                n_dynamic=g.n_dynamic, reader=BGZF_READERS[g.reader], reason=GZIP_REASONS[g.reason], first_bad_item=g.first_bad_item,
                laps_ms=dict(zip(("upload", "sync_count", "decode", "windows", "resolve", "crc"), g.laps_ms)))


class PafInfo(C.Structure):  # include/mahip.h: mahip_paf_info_t
    _fields_ = [("n_lines", C.c_uint64), ("n_records", C.c_uint64), ("n_stored_lines", C.c_uint64), ("n_hits", C.c_uint64), ("name_bytes", C.c_uint64),
                ("n_seq", C.c_uint32), ("max_qs", C.c_uint32), ("n_excl", C.c_uint32)]


class PafReport(C.Structure):  # include/mahip.h: mahip_paf_report_t
    _fields_ = [("n_lines", C.c_uint64), ("n_odd", C.c_uint64), ("n_long", C.c_uint64), ("n_distinct", C.c_uint64),
                ("n_gran", C.c_uint32), ("tile_k", C.c_uint32), ("n_tiles", C.c_uint32), ("n_excl", C.c_uint32),
                ("tile_form", C.c_int), ("open_line", C.c_int), ("odd_ran", C.c_int), ("dict_form", C.c_int), ("bl_pass", C.c_int), ("n_attempts", C.c_int),
                ("cap", C.c_uint32 * 4), ("end", C.c_int * 4)]


class PafStreamReport(C.Structure):  # include/mahip.h: mahip_paf_stream_report_t
    _fields_ = [("n_pieces", C.c_uint64), ("n_empty", C.c_uint64), ("n_short", C.c_uint64), ("n_text", C.c_uint64), ("n_inherited", C.c_uint64),
                ("tab_cap", C.c_uint32), ("n_rebuilds", C.c_uint32), ("n_fold_repeats", C.c_uint32), ("n_rec_grow", C.c_uint32),
                ("last_local", C.c_uint32), ("last_new", C.c_uint32), ("last_before", C.c_uint32), ("last_form", C.c_int),
                ("t_upload", C.c_double), ("t_parse", C.c_double), ("t_fold", C.c_double), ("n_arena_grow", C.c_uint32), ("n_ids_grow", C.c_uint32)]


class PafStreamExclReport(C.Structure):  # include/mahip.h: mahip_paf_stream_excl_report_t
    _fields_ = [("n_early_lines", C.c_uint64), ("n_late_records", C.c_uint64), ("n_late_lines", C.c_uint64), ("peak_records", C.c_uint64),
                ("n_flagged", C.c_uint32), ("n_renumbered", C.c_uint32), ("n_flag_grow", C.c_uint32), ("n_lens_grow", C.c_uint32)]


PAF_DICT_FORMS = {0: None, 1: "short", 2: "text"}  # MAHIP_PAF_DICT_*
PAF_TAB_ENDS = {0: "ok", 1: "load", 2: "probes"}   # MAHIP_PAF_TAB_*


class XferInfo(C.Structure):  # include/mahip.h: mahip_xfer_info_t
    _fields_ = [("road", C.c_int), ("to_device", C.c_int), ("bytes", C.c_uint64), ("slices", C.c_uint64), ("workers", C.c_int)]


XFER_ROADS = {0: None, 1: "runtime", 2: "staged_mem", 3: "staged_file"}  # MAHIP_XFER_*


class TextInfo(C.Structure):  # include/mahip.h: mahip_text_info_t
    _fields_ = [("kind", C.c_int), ("road", C.c_int), ("reason", C.c_int), ("n_records", C.c_uint64), ("n_lines", C.c_uint64), ("text_bytes", C.c_uint64), ("n_slabs", C.c_uint64),
                ("slab_records", C.c_uint64), ("max_name", C.c_uint64), ("n_slow_lines", C.c_uint64), ("laps_ms", C.c_double * 4), ("n_seq_bytes", C.c_uint64),
                ("seq_chunk", C.c_uint64)]


TEXT_KINDS = {"paf": 1, "sg": 2, "bed": 3, "ug": 4}  # MAHIP_TEXT_*
TEXT_ROADS = {0: None, 1: "host", 2: "device"}
TEXT_REASONS = ["OK", "SWITCHED_OFF", "NOMEM", "NO_NAMES", "NO_UG", "NO_SEQ", "SEQ_NUL", "TOO_MANY"]


def _text_dict(t):
    d = {k: getattr(t, k) for k, _ in TextInfo._fields_ if k != "laps_ms"}
    d.update(kind={v: k for k, v in TEXT_KINDS.items()}.get(t.kind), road=TEXT_ROADS.get(t.road), reason=TEXT_REASONS[t.reason], laps_ms=list(t.laps_ms))
    return d


class ProfRec(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_uint64), ("total_ms", C.c_double), ("alg_bytes", C.c_double)]


def build(verbose=False):
    """Compile every HIP and C source in-tree (hipcc --offload-arch=gfx950; works without a GPU)."""
    cmd = ["make", "-C", ROOT, "-j8", "all"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout)
    if r.returncode != 0:
        raise RuntimeError("miniasm_amd build failed")


_lib = None


def lib():
    """The product library.  Raises if it has not been built; never substitutes anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libminiasm_amd.so is not built (run `make` or __graft_entry__.build()); there is no fallback path")
        L = C.CDLL(LIB_PATH)
        vp, sz, u32, i32 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int
        L.mahip_create.restype = vp
        L.mahip_create.argtypes = [i32, vp]
        L.mahip_destroy.argtypes = [vp]
        L.mahip_strerror.restype = C.c_char_p
        L.mahip_device_count.restype = i32
        L.mahip_sync.argtypes = [vp]
        L.mahip_hits_upload.argtypes = [vp, vp, sz, u32]
        L.mahip_hits_adopt.argtypes = [vp, vp, sz, u32]
        L.mahip_set_shard.argtypes = [vp, u32, u32]
        L.mahip_set_hints.argtypes = [vp, u32]
        L.mahip_set_run_stride.argtypes = [vp, i32]
        L.mahip_set_exact_ties.argtypes = [vp, i32]
        L.mahip_tie_stats.argtypes = [vp, C.POINTER(TieInfo)]
        L.mahip_memcpy_h2d.argtypes = [vp, vp, vp, sz]
        L.mahip_memcpy_d2h.argtypes = [vp, vp, vp, sz]
        L.mahip_memcpy_fd2d.argtypes = [vp, vp, i32, sz, sz]
        L.mahip_xfer_last.argtypes = [vp, C.POINTER(XferInfo)]
        L.mahip_scan_u32.argtypes = [vp, vp, vp, sz, vp]
        L.mahip_paf_release.argtypes = [vp]
        L.mahip_hits_sorted_runs.restype = C.c_uint64
        L.mahip_hits_sorted_runs.argtypes = [vp]
        L.mahip_first_launch.argtypes = [vp]
        L.mahip_paf_load_fd.argtypes = [vp, i32, sz]
        L.mahip_paf_load_mem.argtypes = [vp, vp, sz]
        L.mahip_hits_raw_download.argtypes = [vp, vp]
        L.mahip_hits_positions_download.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
        L.mahip_paf_parse_excl.argtypes = [vp, i32, i32, i32, i32, i32, C.c_float, C.POINTER(PafInfo)]
        L.mahip_paf_names.argtypes = [vp, vp, vp]
        L.mahip_paf_last.argtypes = [vp, C.POINTER(PafReport)]
        L.mahip_paf_cols_download.argtypes = [vp] + [vp] * 8
        L.mahip_paf_keep_odd.argtypes = [vp, i32]
        L.mahip_paf_stream_begin.argtypes = [vp, i32, i32, i32]
        L.mahip_paf_stream_begin_excl.argtypes = [vp, i32, i32, i32, i32, i32, C.c_float]
        L.mahip_paf_stream_excl_last.argtypes = [vp, C.POINTER(PafStreamExclReport)]
        L.mahip_paf_stream_piece_mem.argtypes = [vp, vp, sz, i32]
        L.mahip_paf_stream_end.argtypes = [vp, C.POINTER(PafInfo)]
        L.mahip_paf_stream_abort.argtypes = [vp]
        L.mahip_paf_stream_last.argtypes = [vp, C.POINTER(PafStreamReport)]
        L.mahip_paf_stream_tab_download.argtypes = [vp, vp]
        L.mahip_hits_sort.argtypes = [vp]
        L.mahip_hits_index.argtypes = [vp]
        L.mahip_hits_sub.argtypes = [vp, i32, C.c_float, i32, i32, C.POINTER(sz)]
        L.mahip_hits_cut.argtypes = [vp, i32, i32, C.POINTER(sz)]
        L.mahip_hits_flt.argtypes = [vp, i32, i32, i32, C.POINTER(sz), C.POINTER(C.c_float)]
        L.mahip_sub_merge.argtypes = [vp]
        L.mahip_hits_cutflt_sub.argtypes = [vp, i32, i32, i32, i32, i32, C.c_float, i32, i32, C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_float), C.POINTER(sz)]
        L.mahip_hits_cut_contained.argtypes = [vp, i32, i32, C.POINTER(MaOpt), C.POINTER(sz), C.POINTER(u32)]
        L.mahip_hits_contained.argtypes = [vp, C.POINTER(MaOpt), vp, C.POINTER(u32), C.POINTER(sz)]
        L.mahip_sub_upload.argtypes = [vp, i32, vp, sz]
        L.mahip_sub_download.argtypes = [vp, i32, vp, i32]
        L.mahip_seqdel_download.argtypes = [vp, vp]
        L.mahip_map_download.argtypes = [vp, vp]
        L.mahip_hits_live.restype = sz
        L.mahip_hits_live.argtypes = [vp]
        L.mahip_hits_download.argtypes = [vp, vp, C.POINTER(sz)]
        L.mahip_sg_gen.argtypes = [vp, C.POINTER(MaOpt), i32, vp, vp, C.POINTER(u32)]
        L.mahip_asg_upload.argtypes = [vp, C.POINTER(Asg)]
        L.mahip_asg_del_trans.argtypes = [vp, i32, C.POINTER(u32)]
        L.mahip_asg_symm.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.mahip_asg_del_short.argtypes = [vp, C.c_float, C.POINTER(u32)]
        L.mahip_asg_n_arc.restype = u32
        L.mahip_asg_n_arc.argtypes = [vp]
        L.mahip_asg_download.argtypes = [vp, C.POINTER(Asg)]
        L.mahip_prof_enable.argtypes = [vp, i32]
        L.mahip_prof_reset.argtypes = [vp]
        L.mahip_prof_get.argtypes = [vp, C.POINTER(ProfRec), i32]
        L.mahip_mem_bytes.restype = sz
        L.mahip_mem_bytes.argtypes = [vp]
        L.mahip_fastx_load_mem.argtypes = [vp, vp, sz]
        L.mahip_fastx_load_fd.argtypes = [vp, i32, sz]
        L.mahip_fastx_index.argtypes = [vp, C.POINTER(FastxInfo)]
        L.mahip_fastx_release.argtypes = [vp]
        L.mahip_fastx_line_starts.argtypes = [vp, vp]
        L.mahip_fastx_name_spans.argtypes = [vp, vp, vp]
        L.mahip_useq_begin.argtypes = [vp, sz]
        L.mahip_useq_end.argtypes = [vp, vp]
        L.mahip_useq_place_text.argtypes = [vp, vp, sz, vp, sz, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
        L.mahip_useq_last.argtypes = [vp, C.POINTER(UseqInfo)]
        L.mahip_useq_stream_begin.argtypes = [vp, vp, sz, vp, sz]
        L.mahip_useq_stream_piece_mem.argtypes = [vp, vp, sz, i32, C.POINTER(UseqStreamVerdict)]
        L.mahip_useq_stream_window_download.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
        L.mahip_useq_stream_end.argtypes = [vp]
        L.mahip_useq_stream_abort.argtypes = [vp]
        L.mahip_useq_stream_last.argtypes = [vp, C.POINTER(UseqStreamReport)]
        L.mahip_useq_plan.argtypes = [vp, i32, C.POINTER(UseqPlanInfo)]
        L.mahip_useq_plan_mem.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, vp, C.POINTER(UseqPlanInfo)]
        L.mahip_useq_plan_last.argtypes = [vp, C.POINTER(UseqPlanInfo)]
        L.mahip_useq_plan_download.argtypes = [vp, vp, vp, vp, vp]
        L.mahip_useq_begin_planned.argtypes = [vp]
        L.mahip_useq_place_text_planned.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
        L.mahip_useq_stream_begin_planned.argtypes = [vp]
        L.mahip_bgzf_load_fd.argtypes = [vp, i32, sz, i32, C.POINTER(BgzfInfo)]
        L.mahip_bgzf_load_mem.argtypes = [vp, vp, sz, i32, C.POINTER(BgzfInfo)]
        L.mahip_bgzf_inflate_mem.argtypes = [vp, vp, sz, vp, sz, C.POINTER(BgzfInfo)]
        L.mahip_bgzf_last.argtypes = [vp, C.POINTER(BgzfInfo)]
        L.mahip_bgzf_load_fd_range.argtypes = [vp, i32, sz, i32, i32, C.POINTER(BgzfRange), C.POINTER(BgzfInfo)]
        L.mahip_bgzf_range_mem.argtypes = [vp, vp, sz, i32, i32, vp, sz, C.POINTER(BgzfRange), C.POINTER(BgzfInfo)]
        L.mahip_text_first_nl.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
        L.mahip_bgzf_reason_name.restype = C.c_char_p
        L.mahip_bgzf_reason_name.argtypes = [i32]
        L.mahip_gzip_load_fd.argtypes = [vp, i32, sz, i32, sz, C.POINTER(GzipInfo)]
        L.mahip_gzip_load_mem.argtypes = [vp, vp, sz, i32, sz, C.POINTER(GzipInfo)]
        L.mahip_gzip_inflate_mem.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(GzipInfo)]
        L.mahip_gzip_last.argtypes = [vp, C.POINTER(GzipInfo)]
        L.mahip_gzip_load_fd_members.argtypes = [vp, i32, sz, i32, sz, C.POINTER(GzipInfo)]
        L.mahip_gzip_load_mem_members.argtypes = [vp, vp, sz, i32, sz, C.POINTER(GzipInfo)]
        L.mahip_gzip_inflate_mem_members.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(GzipInfo)]
        L.mahip_gzip_members_last.argtypes = [vp, C.POINTER(GzipMembersInfo)]
        L.mahip_gzip_members_download.restype = C.c_uint64
        L.mahip_gzip_members_download.argtypes = [vp, C.POINTER(GzipMember), C.c_uint64]
        L.mahip_gzip_reason_name.restype = C.c_char_p
        L.mahip_gzip_reason_name.argtypes = [i32]
        L.mahip_gzip_items_download.restype = C.c_uint64
        L.mahip_gzip_items_download.argtypes = [vp, C.POINTER(GzipItem), C.c_uint64]
        L.mahip_text_format_mem.argtypes = [vp, i32, vp, C.c_uint64, vp, u32, vp, vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(sz), C.POINTER(TextInfo)]
        L.mahip_text_last.argtypes = [vp, C.POINTER(TextInfo)]
        L.mahip_text_format_ug_mem.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, u32, vp, vp, u32, i32, vp, C.c_uint64, vp, vp, C.c_uint64, C.POINTER(vp), C.POINTER(sz), C.POINTER(TextInfo)]
        L.mahip_scan_forms.argtypes = [vp, C.POINTER(C.c_uint64 * 3)]
        L.mahip_scan_forms.restype = None
        L.ma_opt_init.argtypes = [C.POINTER(MaOpt)]
        L.sd_init.restype = C.POINTER(Sdict)
        L.sd_destroy.argtypes = [C.POINTER(Sdict)]
        L.ma_hit_ingest.restype = vp
        L.ma_hit_ingest.argtypes = [C.c_char_p, i32, i32, C.POINTER(Sdict), C.POINTER(sz), i32, vp]
        L.ma_pipeline_device_mem.restype = i32
        L.ma_pipeline_device_mem.argtypes = [vp, C.POINTER(MaOpt), C.POINTER(Sdict), C.c_char_p, i32, i32, C.POINTER(vp), C.POINTER(sz)]
        L.ma_set_log_path.argtypes = [C.c_char_p]
        L.sys_init.argtypes = []
        L.free_buf = C.CDLL(None).free
        L.free_buf.argtypes = [vp]
        _lib = L
    return _lib


def default_opt():
    o = MaOpt()
    lib().ma_opt_init(C.byref(o))
    return o


class GpuError(RuntimeError):
    pass


def _chk(rc, what):
    if rc != 0:
        raise GpuError("%s failed: %s" % (what, lib().mahip_strerror().decode()))


class Ctx:
    """One GPU context (include/mahip.h).  Construction fails loudly when no GPU is usable."""

    def __init__(self, device=0, stream=None):
        L = lib()
        self.h = L.mahip_create(device, stream)
        if not self.h:
            raise GpuError(L.mahip_strerror().decode())

    def close(self):
        if self.h:
            lib().mahip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_exact_ties(self, mode):
        lib().mahip_set_exact_ties(self.h, mode)

    def tie_stats(self):
        t = TieInfo()
        lib().mahip_tie_stats(self.h, C.byref(t))
        return {k: getattr(t, k) for k, _ in TieInfo._fields_}

    # ---- hits
    def hits_upload(self, hits, n_seq):
        hits = np.ascontiguousarray(hits, dtype=HIT_DT)
        self._keep = hits
        _chk(lib().mahip_hits_upload(self.h, hits.ctypes.data, len(hits), n_seq), "hits_upload")
        _chk(lib().mahip_sync(self.h), "sync")

    def set_run_stride(self, stride):
        """hint for the sort (include/mahip.h): 2 = records and mirrors side by side, 1 = no mirrors, 0 = unknown; describes one upload"""
        _chk(lib().mahip_set_run_stride(self.h, int(stride)), "set_run_stride")

    def hits_adopt(self, dptr, n, n_seq):
        _chk(lib().mahip_hits_adopt(self.h, dptr, n, n_seq), "hits_adopt")

    def paf_stream_last(self):
        r = PafStreamReport()
        _chk(lib().mahip_paf_stream_last(self.h, C.byref(r)), "paf_stream_last")
        return r

    def paf_stream_excl_last(self):
        r = PafStreamExclReport()
        _chk(lib().mahip_paf_stream_excl_last(self.h, C.byref(r)), "paf_stream_excl_last")
        return r

    def paf_stream(self, pieces, min_span, min_match, bi_dir, each=None, no_cont=None):
        """pieces (bytes objects, whole lines each; only the last may end without a newline) through the streamed ingest: begin, a piece at a time, end.
        Returns (PafInfo, PafStreamReport); the context is left as after mahip_paf_parse on the concatenated text.  each(k, report): called behind piece k.
        no_cont=(max_hang, int_frac): -R, the context is left as after mahip_paf_parse_excl (paf_stream_excl_last() has that part's report).
        An error aborts the stream before it is raised."""
        L = lib()
        pieces = list(pieces)
        if no_cont is None:
            _chk(L.mahip_paf_stream_begin(self.h, min_span, min_match, 1 if bi_dir else 0), "paf_stream_begin")
        else:
            _chk(L.mahip_paf_stream_begin_excl(self.h, min_span, min_match, 1 if bi_dir else 0, 1, int(no_cont[0]), float(no_cont[1])), "paf_stream_begin_excl")
        info = PafInfo()
        try:
            for k, p in enumerate(pieces):
                buf = C.create_string_buffer(bytes(p), len(p)) if len(p) else None
                _chk(L.mahip_paf_stream_piece_mem(self.h, buf, len(p), 1 if k + 1 == len(pieces) else 0), "paf_stream_piece_mem")
                if each is not None:
                    each(k, self.paf_stream_last())
            _chk(L.mahip_paf_stream_end(self.h, C.byref(info)), "paf_stream_end")
        except Exception:
            L.mahip_paf_stream_abort(self.h)
            raise
        return info, self.paf_stream_last()

    def sort(self):
        _chk(lib().mahip_hits_sort(self.h), "hits_sort")

    def sorted_runs(self):
        """elements of the last sort if it sorted RUNS of records (hits.hip), else 0: lets a test say which path it took"""
        return int(lib().mahip_hits_sorted_runs(self.h))

    def index(self):
        _chk(lib().mahip_hits_index(self.h), "hits_index")

    def sub(self, min_dp, min_iden, end_clip, slot=0):
        n = C.c_size_t(0)
        _chk(lib().mahip_hits_sub(self.h, min_dp, min_iden, end_clip, slot, C.byref(n)), "hits_sub")
        return n.value

    def cut(self, slot, min_span):
        n = C.c_size_t(0)
        _chk(lib().mahip_hits_cut(self.h, slot, min_span, C.byref(n)), "hits_cut")
        return n.value

    def flt(self, slot, max_hang, min_ovlp):
        n = C.c_size_t(0)
        cov = C.c_float(0)
        _chk(lib().mahip_hits_flt(self.h, slot, max_hang, min_ovlp, C.byref(n), C.byref(cov)), "hits_flt")
        return n.value, cov.value

    def sub_merge(self):
        _chk(lib().mahip_sub_merge(self.h), "sub_merge")

    def cutflt_sub(self, cut_slot, min_span, max_hang, min_ovlp, min_dp, min_iden, end_clip, out_slot):
        """fused: cut against cut_slot + filter inside the coverage pass that writes out_slot -> (n_cut, n_flt, cov, n_remained)"""
        nc, nf, nr = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        cov = C.c_float(0)
        _chk(lib().mahip_hits_cutflt_sub(self.h, cut_slot, min_span, max_hang, min_ovlp, min_dp, min_iden, end_clip, out_slot,
                                         C.byref(nc), C.byref(nf), C.byref(cov), C.byref(nr)), "hits_cutflt_sub")
        return nc.value, nf.value, cov.value, nr.value

    def cut_contained(self, cut_slot, min_span, opt):
        """fused: cut against cut_slot + the flag pass of contained (squeeze of the hits deferred) -> (n_cut, n_seq_new)"""
        n = C.c_size_t(0)
        r = C.c_uint32(0)
        _chk(lib().mahip_hits_cut_contained(self.h, cut_slot, min_span, C.byref(opt), C.byref(n), C.byref(r)), "hits_cut_contained")
        return n.value, r.value

    def contained(self, opt, seq_del=None):
        n = C.c_size_t(0)
        r = C.c_uint32(0)
        p = seq_del.ctypes.data if seq_del is not None else None
        _chk(lib().mahip_hits_contained(self.h, C.byref(opt), p, C.byref(r), C.byref(n)), "hits_contained")
        return r.value, n.value

    def sub_upload(self, slot, sub):
        sub = np.ascontiguousarray(sub, dtype=SUB_DT)
        _chk(lib().mahip_sub_upload(self.h, slot, sub.ctypes.data, len(sub)), "sub_upload")

    def sub_download(self, slot, n, squeezed=False):
        out = np.zeros(n, dtype=SUB_DT)
        _chk(lib().mahip_sub_download(self.h, slot, out.ctypes.data, 1 if squeezed else 0), "sub_download")
        return out

    def seqdel_download(self, n):
        out = np.zeros(n, dtype=np.uint8)
        _chk(lib().mahip_seqdel_download(self.h, out.ctypes.data), "seqdel_download")
        return out

    def map_download(self, n):
        out = np.zeros(n, dtype=np.int32)
        _chk(lib().mahip_map_download(self.h, out.ctypes.data), "map_download")
        return out

    def hits_download(self):
        n = lib().mahip_hits_live(self.h)
        out = np.zeros(max(n, 1), dtype=HIT_DT)
        m = C.c_size_t(0)
        _chk(lib().mahip_hits_download(self.h, out.ctypes.data, C.byref(m)), "hits_download")
        return out[:m.value]

    # ---- graph
    def sg_gen(self, opt, use_sub=True, seq_len=None, seq_del=None):
        n = C.c_uint32(0)
        pl = seq_len.ctypes.data if seq_len is not None else None
        pd = seq_del.ctypes.data if seq_del is not None else None
        _chk(lib().mahip_sg_gen(self.h, C.byref(opt), 1 if use_sub else 0, pl, pd, C.byref(n)), "sg_gen")
        return n.value

    def del_trans(self, fuzz):
        n = C.c_uint32(0)
        _chk(lib().mahip_asg_del_trans(self.h, fuzz, C.byref(n)), "asg_del_trans")
        return n.value

    def symm(self):
        a, b = C.c_uint32(0), C.c_uint32(0)
        _chk(lib().mahip_asg_symm(self.h, C.byref(a), C.byref(b)), "asg_symm")
        return a.value, b.value

    def del_short(self, ratio):
        n = C.c_uint32(0)
        _chk(lib().mahip_asg_del_short(self.h, ratio, C.byref(n)), "asg_del_short")
        return n.value

    def asg_download(self):
        """-> (arcs[ARC_DT], seq[u4], idx[u8]) copies; frees the C arrays."""
        g = Asg()
        _chk(lib().mahip_asg_download(self.h, C.byref(g)), "asg_download")
        na, ns = g.n_arc, g.n_seq
        arcs = np.frombuffer(C.string_at(g.arc, na * 16), dtype=ARC_DT).copy() if na else np.zeros(0, ARC_DT)
        seq = np.frombuffer(C.string_at(g.seq, ns * 4), dtype="<u4").copy() if ns else np.zeros(0, "<u4")
        idx = np.frombuffer(C.string_at(g.idx, ns * 16), dtype="<u8").copy() if ns else np.zeros(0, "<u8")
        for p in (g.arc, g.seq, g.idx):
            lib().free_buf(p)
        return arcs, seq, idx

    # ---- the reads file as text (csrc/useq.hip): for stage tests
    def fastx_load(self, text):
        """a FASTA/FASTQ text (bytes) into HBM"""
        _chk(lib().mahip_fastx_load_mem(self.h, text, len(text)), "fastx_load_mem")

    def fastx_index(self):
        """line index + form check -> dict(format, n_lines, n_records, n_cr, regular, reason) with format / reason as names"""
        fi = FastxInfo()
        _chk(lib().mahip_fastx_index(self.h, C.byref(fi)), "fastx_index")
        return dict(format=FASTX_FORMATS[fi.format], n_lines=fi.n_lines, n_records=fi.n_records, n_cr=fi.n_cr, regular=bool(fi.regular), reason=FASTX_REASONS[fi.reason])

    def fastx_line_starts(self, n_lines):
        out = np.zeros(n_lines + 1, dtype=np.uint64)
        _chk(lib().mahip_fastx_line_starts(self.h, out.ctypes.data), "fastx_line_starts")
        return out

    def fastx_names(self, text, n_records):
        """the records' names as the device delimits them, cut out of `text` (the bytes that were loaded)"""
        off, ln = np.zeros(max(n_records, 1), dtype=np.uint64), np.zeros(max(n_records, 1), dtype=np.uint32)
        _chk(lib().mahip_fastx_name_spans(self.h, off.ctypes.data, ln.ctypes.data), "fastx_name_spans")
        return [text[int(o):int(o) + int(l)] for o, l in zip(off[:n_records], ln[:n_records])]

    def fastx_release(self):
        _chk(lib().mahip_fastx_release(self.h), "fastx_release")

    def useq_place_text(self, arena_bytes, wanted):
        """wanted: dicts(name, dst_off, len, rev, s, e) with e = None for the whole record -> (arena bytes, n_matched, n_dup, n_short);
        the text must be loaded and indexed (regular)"""
        L = lib()
        arr = (UseqWant * max(len(wanted), 1))()
        blob = b""
        for k, w in enumerate(wanted):
            arr[k] = UseqWant(w["dst_off"], len(blob), len(w["name"]), w["len"], w.get("s") or 0, w["e"] if w.get("e") is not None else 0, 1 if w["rev"] else 0, 1 if w.get("e") is None else 0)
            blob += w["name"]
        _chk(L.mahip_useq_begin(self.h, arena_bytes), "useq_begin")
        nm, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _chk(L.mahip_useq_place_text(self.h, C.addressof(arr), len(wanted), blob, len(blob), C.byref(nm), C.byref(nd), C.byref(ns), None), "useq_place_text")
        out = C.create_string_buffer(max(arena_bytes, 1))
        _chk(L.mahip_useq_end(self.h, out), "useq_end")
        return out.raw[:arena_bytes], nm.value, nd.value, ns.value

    # ---- the reads file a piece at a time (csrc/useq.hip): for stage tests
    def useq_stream_last(self):
        """dict of mahip_useq_stream_report_t, format and refused_reason as names"""
        r = UseqStreamReport()
        _chk(lib().mahip_useq_stream_last(self.h, C.byref(r)), "useq_stream_last")
        return dict(format=FASTX_FORMATS[r.format], pieces=r.n_pieces, records=r.n_records, matched=r.n_matched, dup=r.n_dup, short=r.n_short, jobs=r.n_jobs, max_carry=r.max_carry,
                    window_growths=r.n_window_grow, refused_piece=r.refused_piece, refused_reason=FASTX_REASONS[r.refused_reason], laps_ms=list(r.laps_ms))

    def useq_stream_piece(self, text, last):
        """one piece into the open stream -> verdict dict(reason, records, consumed, carry, placed); raises when the stream takes no piece"""
        v = UseqStreamVerdict()
        buf = C.create_string_buffer(bytes(text), len(text)) if len(text) else None
        _chk(lib().mahip_useq_stream_piece_mem(self.h, buf, len(text), 1 if last else 0, C.byref(v)), "useq_stream_piece_mem")
        return dict(reason=FASTX_REASONS[v.reason], records=v.n_records, consumed=v.bytes_consumed, carry=v.carry_bytes, placed=v.n_placed)

    def useq_stream(self, pieces, arena_bytes, wanted, each=None):
        """pieces (bytes objects of whole lines; only the last may end without a newline) through the streamed reader: useq_begin, stream_begin, a piece at a time
        until the last piece or the first verdict other than OK, useq_end.  wanted: as useq_place_text.  each(k, verdict): called behind piece k.
        Returns (arena bytes, or None when arena_bytes is 0; the verdicts; the report).  After a refusal the stream is left open, for useq_stream_window() and
        useq_stream_abort(); otherwise it is ended."""
        L = lib()
        pieces = list(pieces)
        arr = (UseqWant * max(len(wanted), 1))()
        blob = b""
        for k, w in enumerate(wanted):
            arr[k] = UseqWant(w["dst_off"], len(blob), len(w["name"]), w["len"], w.get("s") or 0, w["e"] if w.get("e") is not None else 0, 1 if w["rev"] else 0, 1 if w.get("e") is None else 0)
            blob += w["name"]
        _chk(L.mahip_fastx_release(self.h), "fastx_release")  # (a window buffer of the size the pieces ask for: the growths are the stream's own)
        _chk(L.mahip_useq_begin(self.h, arena_bytes), "useq_begin")
        _chk(L.mahip_useq_stream_begin(self.h, C.addressof(arr), len(wanted), blob, len(blob)), "useq_stream_begin")
        return self._useq_stream_pieces(pieces, arena_bytes, each)

    def _useq_stream_pieces(self, pieces, arena_bytes, each):
        """the pieces through the stream that was begun, then the arena"""
        L = lib()
        verdicts = []
        try:
            for k, p in enumerate(pieces):
                verdicts.append(self.useq_stream_piece(p, k + 1 == len(pieces)))
                if each is not None:
                    each(k, verdicts[-1])
                if verdicts[-1]["reason"] != "OK":
                    break
            else:
                _chk(L.mahip_useq_stream_end(self.h), "useq_stream_end")
        except Exception:
            L.mahip_useq_stream_abort(self.h)
            raise
        out = C.create_string_buffer(max(arena_bytes, 1))
        _chk(L.mahip_useq_end(self.h, out), "useq_end")
        return (out.raw[:arena_bytes] if arena_bytes else None), verdicts, self.useq_stream_last()

    def useq_stream_window(self):
        """after a verdict other than OK: the bytes of the refused window (carry + piece)"""
        n = C.c_uint64(0)
        _chk(lib().mahip_useq_stream_window_download(self.h, None, C.byref(n)), "useq_stream_window_download")
        buf = C.create_string_buffer(max(n.value, 1))
        _chk(lib().mahip_useq_stream_window_download(self.h, buf, C.byref(n)), "useq_stream_window_download")
        return buf.raw[:n.value]

    def useq_stream_abort(self):
        _chk(lib().mahip_useq_stream_abort(self.h), "useq_stream_abort")

    # ---- the placement plan on the device (csrc/useq.hip): for stage tests
    def useq_plan_mem(self, units, names, sub=None):
        """hand-made unitigs planned on the device.  units: one (len, start, end, members) per unitig as text_format_ug takes them (start / end are not looked at);
        names: one bytes object per read, or None (no names: the plan refuses); sub: SUB_DT per read or None.  Returns the info dict (useq_plan_last)"""
        U = len(units)
        u_len = np.array([u[0] for u in units], dtype=np.uint32)
        u_n = np.array([len(u[3]) for u in units], dtype=np.uint32)
        mem = np.array([m for u in units for m in u[3]], dtype=np.uint64)
        if names is not None:
            n_seq = len(names)
            off = np.zeros(n_seq + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
            blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        else:
            n_seq = 0 if sub is None else len(sub)
        sub = None if sub is None else np.ascontiguousarray(sub, dtype=SUB_DT)
        assert sub is None or len(sub) == n_seq
        info = UseqPlanInfo()
        _chk(lib().mahip_useq_plan_mem(self.h, U, u_n.ctypes.data, u_len.ctypes.data, mem.ctypes.data, n_seq, None if names is None else blob.ctypes.data,
                                       None if names is None else off.ctypes.data, None if sub is None else sub.ctypes.data, C.byref(info)), "useq_plan_mem")
        return _plan_dict(info)

    def useq_plan_last(self):
        """the info of the context's last placement plan (a refused one included): road, reason, n_utg, n_members, n_reads, n_wanted, name_bytes, blob_bytes,
        arena_bytes, n_multi, uoff_tiles, ms"""
        p = UseqPlanInfo()
        _chk(lib().mahip_useq_plan_last(self.h, C.byref(p)), "useq_plan_last")
        return _plan_dict(p)

    def useq_plan_download(self):
        """the plan the context holds -> (uoff [n_utg + 1] u64, per-read plan PLACE_DT, wanted table WANT_DT, the blob its name_off point into)"""
        p = self.useq_plan_last()
        uoff = np.zeros(p["n_utg"] + 1, dtype=np.uint64)
        pl = np.zeros(max(p["n_reads"], 1), dtype=PLACE_DT)
        want = np.zeros(max(p["n_wanted"], 1), dtype=WANT_DT)
        names = C.create_string_buffer(max(p["blob_bytes"], 1))
        _chk(lib().mahip_useq_plan_download(self.h, uoff.ctypes.data, pl.ctypes.data, want.ctypes.data, names), "useq_plan_download")
        return uoff, pl[:p["n_reads"]], want[:p["n_wanted"]], names.raw[:p["blob_bytes"]]

    def useq_place_text_planned(self):
        """useq_place_text with the arena and the wanted table of the plan the context holds -> (arena bytes, n_matched, n_dup, n_short)"""
        L = lib()
        arena_bytes = self.useq_plan_last()["arena_bytes"]
        _chk(L.mahip_useq_begin_planned(self.h), "useq_begin_planned")
        nm, nd, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _chk(L.mahip_useq_place_text_planned(self.h, C.byref(nm), C.byref(nd), C.byref(ns), None), "useq_place_text_planned")
        out = C.create_string_buffer(max(arena_bytes, 1))
        _chk(L.mahip_useq_end(self.h, out), "useq_end")
        return out.raw[:arena_bytes], nm.value, nd.value, ns.value

    def useq_stream_planned(self, pieces, each=None):
        """useq_stream with the arena and the wanted table of the plan the context holds"""
        L = lib()
        arena_bytes = self.useq_plan_last()["arena_bytes"]
        _chk(L.mahip_fastx_release(self.h), "fastx_release")
        _chk(L.mahip_useq_begin_planned(self.h), "useq_begin_planned")
        _chk(L.mahip_useq_stream_begin_planned(self.h), "useq_stream_begin_planned")
        return self._useq_stream_pieces(list(pieces), arena_bytes, each)

    def useq_last(self):
        """which reader the context's last ma_ug_seq used, and why"""
        u = UseqInfo()
        _chk(lib().mahip_useq_last(self.h, C.byref(u)), "useq_last")
        return dict(reader=USEQ_READERS[u.reader], reason=FASTX_REASONS[u.reason], format=FASTX_FORMATS[u.format], n_records=u.n_records, n_matched=u.n_matched, n_dup=u.n_dup, n_short=u.n_short)

    # ---- bgzip-compressed input inflated on the device (csrc/xfer.hip, csrc/inflate_core.h)
    def bgzf_inflate(self, comp, out_cap=None):
        """a BGZF image (bytes) -> (text, info dict); text is None when the device refused it (info["reason"] says why) -- nothing stays loaded either way"""
        bi = BgzfInfo()
        cap = out_cap if out_cap is not None else 65536 * (len(comp) // 28 + 1)  # a member is at least 28 bytes and holds at most 64 KiB
        out = C.create_string_buffer(max(cap, 1))
        _chk(lib().mahip_bgzf_inflate_mem(self.h, comp, len(comp), out, cap, C.byref(bi)), "bgzf_inflate_mem")
        info = _bgzf_dict(bi)
        return (out.raw[:bi.text_bytes] if info["reason"] == "OK" else None), info

    def bgzf_load(self, comp, target="paf"):
        """a BGZF image into the text buffer of the PAF reader or of the reads-file reader, as mahip_paf_load_mem / mahip_fastx_load_mem leave it -> info dict"""
        bi = BgzfInfo()
        _chk(lib().mahip_bgzf_load_mem(self.h, comp, len(comp), BGZF_TARGETS[target], C.byref(bi)), "bgzf_load_mem")
        return _bgzf_dict(bi)

    def bgzf_range(self, comp, rank, world, out_cap=None):
        """a BGZF image (bytes) -> (the text of rank `rank` of `world`, range dict, info dict): only the members that hold the rank's range are inflated; text is
        None when the device refused them -- nothing stays loaded either way"""
        bi, rg = BgzfInfo(), BgzfRange()
        cap = out_cap if out_cap is not None else 65536 * (len(comp) // 28 + 1)
        out = C.create_string_buffer(max(cap, 1))
        _chk(lib().mahip_bgzf_range_mem(self.h, comp, len(comp), rank, world, out, cap, C.byref(rg), C.byref(bi)), "bgzf_range_mem")
        info = _bgzf_dict(bi)
        return (out.raw[:rg.end - rg.beg] if info["reason"] == "OK" else None), _bgzf_range_dict(rg), info

    def bgzf_load_range(self, fd, nbytes, rank, world):
        """the rank's range of an open BGZF overlap file into the text buffer of the PAF reader, as mahip_paf_load_fd_range leaves it on the inflated file
        -> (range dict, info dict)"""
        bi, rg = BgzfInfo(), BgzfRange()
        _chk(lib().mahip_bgzf_load_fd_range(self.h, fd, nbytes, rank, world, C.byref(rg), C.byref(bi)), "bgzf_load_fd_range")
        return _bgzf_range_dict(rg), _bgzf_dict(bi)

    def text_first_nl(self, dptr, lo, hi):
        """for stage tests: the position of the first newline among the bytes [lo, hi) of the device text at dptr (an int), None when there is none"""
        pos = C.c_uint64(0)
        _chk(lib().mahip_text_first_nl(self.h, dptr, lo, hi, C.byref(pos)), "text_first_nl")
        return None if pos.value == 2 ** 64 - 1 else pos.value

    def bgzf_last(self):
        """what the context's last BGZF load decided"""
        bi = BgzfInfo()
        _chk(lib().mahip_bgzf_last(self.h, C.byref(bi)), "bgzf_last")
        return _bgzf_dict(bi)

    # ---- plain gzip input inflated on the device (csrc/xfer.hip: k_gz_*, csrc/gzip_core.h)
    def gzip_inflate(self, comp, chunk=None, out_cap=None, members=False):
        """a gzip image (bytes) -> (text, info dict); text is None when the device refused it (info["reason"] says why); chunk: bytes of payload per chunk (None:
        MA_GZIP_CHUNK or the default) -- nothing stays loaded either way.  members: concatenated members are one text (else a second member is MULTI_MEMBER)"""
        gi = GzipInfo()
        cap = out_cap if out_cap is not None else 1032 * len(comp) + 64  # deflate's best ratio
        out = C.create_string_buffer(max(cap, 1))
        fn = lib().mahip_gzip_inflate_mem_members if members else lib().mahip_gzip_inflate_mem
        _chk(fn(self.h, comp, len(comp), chunk or 0, out, cap, C.byref(gi)), "gzip_inflate_mem")
        info = _gzip_dict(gi)
        return (out.raw[:gi.text_bytes] if info["reason"] == "OK" else None), info

    def gzip_load(self, comp, target="paf", chunk=None, members=False):
        """a gzip image into the text buffer of the PAF reader or of the reads-file reader, as mahip_paf_load_mem / mahip_fastx_load_mem leave it -> info dict"""
        gi = GzipInfo()
        fn = lib().mahip_gzip_load_mem_members if members else lib().mahip_gzip_load_mem
        _chk(fn(self.h, comp, len(comp), BGZF_TARGETS[target], chunk or 0, C.byref(gi)), "gzip_load_mem")
        return _gzip_dict(gi)

    def gzip_members_info(self):
        """the member facts of the last plain-gzip load: dict(n_members, n_candidates, n_heads, bad_member (-1: none), cand_cap, laps_ms)"""
        mi = GzipMembersInfo()
        _chk(lib().mahip_gzip_members_last(self.h, C.byref(mi)), "gzip_members_last")
        return dict(n_members=mi.n_members, n_candidates=mi.n_candidates, n_heads=mi.n_heads, bad_member=mi.bad_member, cand_cap=mi.cand_cap, laps_ms=dict(zip(("scan", "heads"), mi.laps_ms)))

    def gzip_members(self):
        """one row per member of the last load with members=True, in file order: dict(comp_off, hdr_len, text_off, text_len, crc, isize, n_items)"""
        n = self.gzip_members_info()["n_members"]
        rows = (GzipMember * max(n, 1))()
        n = lib().mahip_gzip_members_download(self.h, rows, n)
        return [dict(comp_off=r.comp_off, hdr_len=r.hdr_len, text_off=r.text_off, text_len=r.text_len, crc=r.crc, isize=r.isize, n_items=r.n_items) for r in rows[:n]]

    def gzip_last(self):
        """what the context's last plain-gzip load decided"""
        gi = GzipInfo()
        _chk(lib().mahip_gzip_last(self.h, C.byref(gi)), "gzip_last")
        return _gzip_dict(gi)

    def gzip_items(self):
        """one row per chunk of the last plain-gzip load: dict(sync_bit (None: the chunk found no start), end_bit, out_len, status (a GZIP_REASONS name), saw_final, on_chain)"""
        n = self.gzip_last()["n_chunks"]
        rows = (GzipItem * max(n, 1))()
        n = lib().mahip_gzip_items_download(self.h, rows, n)
        return [dict(sync_bit=None if r.sync_bit < 0 else r.sync_bit, end_bit=r.end_bit, out_len=r.out_len, status=GZIP_REASONS[r.status], saw_final=bool(r.flags & 1), on_chain=bool(r.flags & 2))
                for r in rows[:n]]

    # ---- text of the record dumps (csrc/text_dev.hpp): for stage tests
    def text_format(self, kind, records, names, sub=None, dele=None, slab=None):
        """hand-made records formatted on the device: kind "paf" (records: HIT_DT), "sg" (ARC_DT; sub may be None) or "bed" (records ignored: one line per read);
        names: one bytes object per read; sub: SUB_DT per read; dele: one flag per read (bed); slab: records per slab (None: the default).  Returns (text, info dict)"""
        k = TEXT_KINDS[kind]
        n_seq = len(names)
        off = np.zeros(n_seq + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        if kind == "bed":
            rec, n = None, n_seq
        else:
            rec = np.ascontiguousarray(records, dtype=HIT_DT if kind == "paf" else ARC_DT)
            n = len(rec)
        sub = None if sub is None else np.ascontiguousarray(sub, dtype=SUB_DT)
        assert sub is None or len(sub) == n_seq
        dele = None if dele is None else np.ascontiguousarray(dele, dtype=np.uint8)
        buf, ln, info = C.c_void_p(0), C.c_size_t(0), TextInfo()
        _chk(lib().mahip_text_format_mem(self.h, k, None if rec is None or n == 0 else rec.ctypes.data, n, None if sub is None else sub.ctypes.data, n_seq,
                                         None if dele is None else dele.ctypes.data, blob.ctypes.data, off.ctypes.data, slab or 0, C.byref(buf), C.byref(ln), C.byref(info)), "text_format")
        out = C.string_at(buf, ln.value)
        lib().free_buf(buf)
        return out, _text_dict(info)

    def text_format_ug(self, units, links, counts, names, sub=None, seqs=None, slab=None):
        """hand-made unitigs as a GFA formatted on the device.  units: one (len, start, end, members) per unitig -- start == end == 0xffffffff: circular; members: the
        member words (vertex << 32 | length to the next read); links: ARC_DT records in output order; counts: (arcs leaving end 0, end 1) per unitig; names: one bytes
        object per read; sub: SUB_DT per read or None; seqs: None (S lines carry "*"), or one bytes object per unitig, len(seqs[i]) == units[i][0] -- or a ready arena
        image as one bytes object, or False: sequences are asked for but there is no arena; slab: records per slab (None: the default).
        Returns (text, info dict); text is None when the writer refused (info["road"] == "host", info["reason"] says why)"""
        U, n_seq = len(units), len(names)
        off = np.zeros(n_seq + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        u_len = np.array([u[0] for u in units], dtype=np.uint32)
        u_start = np.array([u[1] for u in units], dtype=np.uint32)
        u_end = np.array([u[2] for u in units], dtype=np.uint32)
        u_n = np.array([len(u[3]) for u in units], dtype=np.uint32)
        mem = np.array([m for u in units for m in u[3]], dtype=np.uint64)
        lk = np.ascontiguousarray(links if links is not None else [], dtype=ARC_DT)
        cnt = np.ascontiguousarray(np.array(counts, dtype=np.uint32).reshape(-1))
        assert len(cnt) == 2 * U
        sub = None if sub is None else np.ascontiguousarray(sub, dtype=SUB_DT)
        assert sub is None or len(sub) == n_seq
        arena = None
        if seqs is not None and seqs is not False:
            img = seqs if isinstance(seqs, (bytes, bytearray)) else b"".join(bytes(x) + b"N" for x in seqs)
            arena = np.frombuffer(bytes(img) + b"\0", dtype=np.uint8)  # (the byte behind the image is never looked at)
            arena_bytes = len(img)
        buf, ln, info = C.c_void_p(0), C.c_size_t(0), TextInfo()
        _chk(lib().mahip_text_format_ug_mem(self.h, U, u_n.ctypes.data, u_len.ctypes.data, u_start.ctypes.data, u_end.ctypes.data, mem.ctypes.data, lk.ctypes.data, len(lk), cnt.ctypes.data,
                                            None if sub is None else sub.ctypes.data, n_seq, 0 if seqs is None else 1, None if arena is None else arena.ctypes.data,
                                            0 if arena is None else arena_bytes, blob.ctypes.data, off.ctypes.data, slab or 0, C.byref(buf), C.byref(ln), C.byref(info)), "text_format_ug")
        d = _text_dict(info)
        if not buf.value:
            return None, d
        out = C.string_at(buf, ln.value)
        lib().free_buf(buf)
        return out, d

    def text_last(self):
        """what the context's last dump through the device text writer did (or why the host formatter ran)"""
        t = TextInfo()
        _chk(lib().mahip_text_last(self.h, C.byref(t)), "text_last")
        return _text_dict(t)

    def scan_forms(self):
        """device-wide scans of this context so far by form: (one tile, chained, three-phase)"""
        out = (C.c_uint64 * 3)()
        lib().mahip_scan_forms(self.h, C.byref(out))
        return tuple(out)

    def scan_u32(self, d_in, d_out, n, d_total=None):
        """for stage tests: the device-wide exclusive scan on device addresses (ints); d_out may equal d_in, d_total may be None.  Queued, not waited for."""
        _chk(lib().mahip_scan_u32(self.h, d_in, d_out, n, d_total), "scan_u32")

    # ---- bulk copies (csrc/xfer.hip): for stage tests
    def memcpy_h2d(self, dptr, host_addr, nbytes):
        return lib().mahip_memcpy_h2d(self.h, dptr, host_addr, nbytes)

    def memcpy_d2h(self, host_addr, dptr, nbytes):
        return lib().mahip_memcpy_d2h(self.h, host_addr, dptr, nbytes)

    def memcpy_fd2d(self, dptr, fd, off, nbytes):
        """bytes [off, off + nbytes) of an open file -> device memory; returns the C return code (-1: the file ended early)"""
        return lib().mahip_memcpy_fd2d(self.h, dptr, fd, off, nbytes)

    def xfer_last(self):
        """what the context's last bulk copy did: dict(road, to_device, bytes, slices, workers)"""
        x = XferInfo()
        _chk(lib().mahip_xfer_last(self.h, C.byref(x)), "xfer_last")
        return dict(road=XFER_ROADS[x.road], to_device=bool(x.to_device), bytes=x.bytes, slices=x.slices, workers=x.workers)

    # ---- instrumentation
    def prof_enable(self, on=True):
        lib().mahip_prof_enable(self.h, 1 if on else 0)

    def prof_reset(self):
        lib().mahip_prof_reset(self.h)

    def prof_get(self):
        buf = (ProfRec * 64)()
        n = lib().mahip_prof_get(self.h, buf, 64)
        return [dict(name=buf[i].name.decode(), launches=buf[i].launches, total_ms=buf[i].total_ms, alg_bytes=buf[i].alg_bytes) for i in range(min(n, 64))]

    def mem_bytes(self):
        return lib().mahip_mem_bytes(self.h)


class Ingest:
    """Host ingest of a PAF file (reference hit.c:70-101, everything before the sort): hits + dictionary."""

    def __init__(self, fn, opt=None, bi_dir=True):
        L = lib()
        opt = opt or default_opt()
        self.d = L.sd_init()
        n = C.c_size_t(0)
        p = L.ma_hit_ingest(fn.encode(), opt.min_span, opt.min_match, self.d, C.byref(n), 1 if bi_dir else 0, None)
        self.n = n.value
        L.ma_ingest_max_qs.restype = C.c_uint32
        self.max_qs = L.ma_ingest_max_qs()  # exact bound of the query starts: hint for the device sort
        self._p = p  # malloc'ed by the library; self.hits is a zero-copy view of it (no second copy of multi-GB arrays)
        if self.n:
            raw = (C.c_uint8 * (self.n * 32)).from_address(p)
            self.hits = np.frombuffer(raw, dtype=HIT_DT)
        else:
            self.hits = np.zeros(0, HIT_DT)
        self.n_seq = self.d.contents.n_seq

    def names(self):
        d = self.d.contents
        return [d.seq[i].name.decode() for i in range(d.n_seq)]

    def lens(self):
        d = self.d.contents
        return np.array([d.seq[i].len for i in range(d.n_seq)], dtype=np.uint32)

    def free_hits(self):
        """release the host copy of the hit records (the dictionary stays)"""
        self.hits = np.zeros(0, HIT_DT)
        if self._p:
            lib().free_buf(self._p)
            self._p = None

    def close(self):
        self.free_hits()
        if self.d:
            lib().sd_destroy(self.d)
            self.d = None


class GpuIngest:
    """Device-side ingest (csrc/paf.hip through host/ingest_gpu.c): the records stay in `ctx`; the dictionary comes back.
    Same attributes as Ingest; `hits` downloads the unsorted records (tests)."""

    def __init__(self, ctx, fn, opt=None, bi_dir=True):
        L = lib()
        opt = opt or default_opt()
        self.ctx = ctx
        self.d = L.sd_init()
        n = C.c_size_t(0)
        L.ma_hit_ingest_gpu.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(Sdict), C.POINTER(C.c_size_t), C.c_int]
        rc = L.ma_hit_ingest_gpu(ctx.h, fn.encode(), opt.min_span, opt.min_match, self.d, C.byref(n), 1 if bi_dir else 0)
        if rc != 0:
            raise OSError("cannot open %s" % fn)
        self.n = n.value
        self.n_seq = self.d.contents.n_seq

    @property
    def hits(self):
        out = np.zeros(self.n, dtype=HIT_DT)
        L = lib()
        L.mahip_hits_raw_download.argtypes = [C.c_void_p, C.c_void_p]
        _chk(L.mahip_hits_raw_download(self.ctx.h, out.ctypes.data), "hits_raw_download")
        return out

    names = Ingest.names
    lens = Ingest.lens

    def close(self):
        if self.d:
            lib().sd_destroy(self.d)
            self.d = None


def run_resident(ctx, opt, ingest, outfmt="ug", stage=100, flags=0):
    """Everything after ingest with the hits resident in HBM (pipeline.c:ma_pipeline_device); returns the output text."""
    L = lib()
    buf = C.c_void_p(0)
    ln = C.c_size_t(0)
    rc = L.ma_pipeline_device_mem(ctx.h, C.byref(opt), ingest.d, outfmt.encode(), stage, flags, C.byref(buf), C.byref(ln))
    if rc != 0:
        raise GpuError("pipeline failed: %s" % L.mahip_strerror().decode())
    out = C.string_at(buf, ln.value)
    L.free_buf(buf)
    return out


def run_resident_handoff(ctx, ctx2, opt, ingest, outfmt="ug", stage=100, flags=0):
    """The same job split over two contexts of one device (include/mahip.h: mahip_tail_handoff): hit passes, graph and reduction on ctx,
    cleaners + unitigs + downloads on ctx2 -- what a caller with a stream of inputs overlaps with the next input's hit passes."""
    L = lib()
    vp = C.c_void_p
    L.ma_pipeline_head.restype = C.c_int
    L.ma_pipeline_head.argtypes = [vp, C.POINTER(MaOpt), C.POINTER(Sdict), C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint32 * 4)]
    L.ma_pipeline_tail_mem.restype = C.c_int
    L.ma_pipeline_tail_mem.argtypes = [vp, C.POINTER(MaOpt), C.POINTER(Sdict), C.c_char_p, C.c_int, C.POINTER(C.c_uint32 * 4), C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.mahip_tail_handoff.argtypes = [vp, vp]
    st = (C.c_uint32 * 4)(0, 0, 0, 0)
    if L.ma_pipeline_head(ctx.h, C.byref(opt), ingest.d, outfmt.encode(), stage, flags, C.byref(st)) != 0:
        raise GpuError("pipeline head failed: %s" % L.mahip_strerror().decode())
    _chk(L.mahip_tail_handoff(ctx.h, ctx2.h), "tail_handoff")
    buf, ln = vp(0), C.c_size_t(0)
    if L.ma_pipeline_tail_mem(ctx2.h, C.byref(opt), ingest.d, outfmt.encode(), stage, C.byref(st), C.byref(buf), C.byref(ln)) != 0:
        raise GpuError("pipeline tail failed: %s" % L.mahip_strerror().decode())
    out = C.string_at(buf, ln.value)
    L.free_buf(buf)
    return out
