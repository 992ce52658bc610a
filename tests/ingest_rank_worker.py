"""One rank of the sharded PAF ingest, case after case, without torch: what ma_hit_ingest_sharded (host/ingest_sharded.c) does through the ABI -- mahip_set_shard,
mahip_paf_load_fd_range, mahip_paf_parse_sharded, mahip_hits_route, mahip_paf_release -- on the byte range the TEST chose for this rank, over the shared-memory
double of the collectives; what the context holds behind the parse and behind the route goes into one .npz per case.  Started by
tests/test_gpu_ingest_shard_edges.py, once per rank: rank, world, segment name, job file (JSON), output directory.  The first call that fails is written down
with the library's message and ends the process with a non-zero status (the parent then ends the other ranks: they would wait for this one for ever)."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if os.environ.get("MA_WORKER_EMU") == "1":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
    import emu_plugin  # noqa: F401
import miniasm_amd as ma  # noqa: E402


def snapshot(L, ctx, min_span, min_match, bi_dir, comm):
    """parse (+ route, with a communicator or without) -> dict of arrays; the calls of host/ingest_sharded.c in their order"""
    vp, u64 = C.c_void_p, C.c_uint64
    out = {}
    info = ma.PafInfo()
    ma._chk(L.mahip_paf_parse_sharded(ctx.h, min_span, min_match, bi_dir, C.byref(info)), "paf_parse_sharded")
    out["info"] = np.array([info.n_lines, info.n_records, info.n_stored_lines, info.n_hits, info.name_bytes, info.n_seq, info.max_qs, info.n_excl], dtype=np.uint64)
    rep = ma.PafReport()
    ma._chk(L.mahip_paf_last(ctx.h, C.byref(rep)), "paf_last")
    n = int(rep.n_lines)
    out["rep"] = np.array([rep.n_lines, rep.bl_pass, rep.dict_form, rep.n_distinct, rep.n_long], dtype=np.uint64)
    flags, nums = np.zeros(max(n, 1), dtype=np.uint8), np.zeros((8, max(n, 1)), dtype=np.uint32)
    ma._chk(L.mahip_paf_cols_download(ctx.h, flags.ctypes.data, None, nums.ctypes.data, None, None, None, None, None), "paf_cols_download")
    out["flags"], out["nums"] = flags[:n], nums[:, :n]
    names = C.create_string_buffer(max(int(info.name_bytes), 1))
    lens = np.zeros(max(int(info.n_seq), 1), dtype=np.uint32)
    ma._chk(L.mahip_paf_names(ctx.h, names, lens.ctypes.data), "paf_names")
    out["names"], out["lens"] = np.frombuffer(names.raw[:int(info.name_bytes)], dtype=np.uint8).copy(), lens[:int(info.n_seq)]
    hits = np.zeros(max(int(info.n_hits), 1), dtype=ma.HIT_DT)
    ma._chk(L.mahip_hits_raw_download(ctx.h, hits.ctypes.data), "hits_raw_download (parse)")
    out["parsed"] = hits[:int(info.n_hits)]
    n_total, sent = u64(0), u64(0)
    ma._chk(L.mahip_hits_route(ctx.h, C.byref(n_total), C.byref(sent)), "hits_route")
    out["route"] = np.array([n_total.value, sent.value], dtype=np.uint64)
    bw = C.c_int(0)
    p = L.mahip_shard_bounds(ctx.h, C.byref(bw))
    out["bounds"] = np.array([int(p[r]) for r in range(bw.value + 1)] if bw.value else [], dtype=np.uint32)
    n_my = int(L.mahip_hits_live(ctx.h))
    assert n_my <= n_total.value, "a rank holds more records than all ranks together"
    hits = np.zeros(max(n_my, 1), dtype=ma.HIT_DT)
    ma._chk(L.mahip_hits_raw_download(ctx.h, hits.ctypes.data), "hits_raw_download (route)")
    out["routed"] = hits[:n_my]
    pos, tot = np.zeros(max(n_my, 1), dtype=np.uint32), u64(0)
    out["have_pos"] = np.array([L.mahip_hits_have_positions(ctx.h)], dtype=np.int64)
    if out["have_pos"][0]:  # (none where the ranks hold no record at all)
        ma._chk(L.mahip_hits_positions_download(ctx.h, pos.ctypes.data, C.byref(tot)), "hits_positions_download")
    out["pos"], out["pos_total"] = pos[:n_my], np.array([tot.value], dtype=np.uint64)
    ma._chk(L.mahip_paf_release(ctx.h), "paf_release")
    return out


def bind(L):
    vp, sz, i32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64
    L.mahip_comm_init_shm.argtypes = [vp, C.c_char_p, i32, i32]
    L.mahip_comm_destroy.argtypes = [vp]
    L.mahip_paf_load_fd_range.argtypes = [vp, i32, sz, sz]
    L.mahip_paf_parse_sharded.argtypes = [vp, i32, i32, i32, C.POINTER(ma.PafInfo)]
    L.mahip_hits_route.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.mahip_shard_bounds.restype = C.POINTER(C.c_uint32)
    L.mahip_shard_bounds.argtypes = [vp, C.POINTER(i32)]
    L.mahip_hits_have_positions.argtypes = [vp]
    return L


def run_case(L, ctx, path, off, nbytes, min_span, min_match, bi_dir, comm):
    ma._chk(L.mahip_set_shard(ctx.h, 0, 0xffffffff), "set_shard")
    fd = os.open(path, os.O_RDONLY)
    try:
        ma._chk(L.mahip_paf_load_fd_range(ctx.h, fd, off, nbytes), "paf_load_fd_range")
    finally:
        os.close(fd)
    return snapshot(L, ctx, min_span, min_match, bi_dir, comm)


def main():
    rank, world, name, job, out_dir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    L = bind(ma.lib())
    L.ma_set_log_path(b"/dev/null")
    with open(job) as f:
        cases = json.load(f)
    ctx = ma.Ctx(0)
    what = "start-up"
    try:
        ma._chk(L.mahip_comm_init_shm(ctx.h, name.encode(), rank, world), "comm_init_shm")
        for case in cases:
            what = case["name"]
            off, nbytes = case["ranges"][rank]
            got = run_case(L, ctx, case["path"], off, nbytes, case["min_span"], case["min_match"], case["bi_dir"], True)
            np.savez(os.path.join(out_dir, "%s.r%d.npz" % (case["name"], rank)), **got)
    except Exception as e:  # no retry, no next case: the other ranks are ended by the parent
        with open(os.path.join(out_dir, "FAILED.r%d" % rank), "w") as f:
            f.write("rank %d of %d, case %s: %s\n" % (rank, world, what, e))
        sys.stderr.write("rank %d of %d, case %s: %s\n" % (rank, world, what, e))
        sys.stderr.flush()
        os._exit(3)
    L.mahip_comm_destroy(ctx.h)
    ctx.close()


if __name__ == "__main__":
    main()
