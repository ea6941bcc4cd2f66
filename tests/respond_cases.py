"""TEST-ONLY: pwaf_respond called through ctypes over guarded blocks, in host memory (numpy) or in device memory (torch), for
tests/test_respond_cpu.py and tests/test_gpu_respond.py. Every output lies in a block filled with 0x5A with GUARD more bytes of 0x5A behind
it: what the call does not write must still read 0x5A, behind each output and inside it (list entries at or past min(n, cap))."""
from __future__ import annotations

import ctypes as C

import numpy as np

import respond_oracle as O
from pingoo_amd import VERDICT_DTYPE, _abi
from pingoo_amd.engine import lib

GUARD = 64
FILL = 0x5A


class HostMem:
    memory = _abi.MEM_HOST

    def block(self, nbytes, init=None):
        raw = np.full(nbytes + GUARD + 16, FILL, dtype=np.uint8)
        at = -raw.ctypes.data % 16
        blk = raw[at:at + nbytes + GUARD]
        if init is not None:
            blk[:nbytes] = np.frombuffer(init, dtype=np.uint8)
        return blk

    def ptr(self, blk):
        return blk.ctypes.data

    def read(self, blk):
        return blk

    def scratch(self, n):
        return None, 0


class DeviceMem:
    memory = _abi.MEM_DEVICE

    def __init__(self, device="cuda:0"):
        import torch

        self.torch, self.device = torch, torch.device(device)

    def block(self, nbytes, init=None):
        host = np.full(nbytes + GUARD, FILL, dtype=np.uint8)
        if init is not None:
            host[:nbytes] = np.frombuffer(init, dtype=np.uint8)
        return self.torch.from_numpy(host).to(self.device)  # (torch's allocations are 256-byte aligned)

    def ptr(self, blk):
        return blk.data_ptr()

    def read(self, blk):
        return blk.cpu().numpy()

    def scratch(self, n):
        need = int(lib().pwaf_respond_scratch_bytes(n))
        blk = self.block(need)
        return blk, need


class Call:
    """One pwaf_respond call over guarded blocks. lists: [tuple of kinds or a mask]; caps: per list (None: n); count_only: the lists whose
    idx is NULL (their cap must be 0). lead / pad: where the first path begins in its arena and how many bytes lie behind the last."""

    def __init__(self, mem, verdicts, statuses, routes, paths, lists=(), caps=None, lead=0, pad=O.ARENA_PAD, with_counts=True, n=None):
        self.mem, self.n = mem, len(verdicts) if n is None else n
        n = self.n
        self.masks = [k if isinstance(k, int) else O.mask_of(k) for k in lists]
        self.caps = [n] * len(lists) if caps is None else list(caps)
        v = np.zeros(max(1, len(verdicts)), dtype=VERDICT_DTYPE)
        if len(verdicts):
            v["action"], v["rule_idx"] = [a for a, _ in verdicts], [r for _, r in verdicts]
        data, off = O.path_column(paths, lead, pad)
        self.keep = [mem.block(v.nbytes, v.tobytes()), mem.block(max(1, len(data)), data.tobytes() or b"\0"), mem.block(off.nbytes, off.tobytes())]
        self.statuses = None if statuses is None else mem.block(max(1, n), np.asarray(list(statuses) or [0], dtype=np.uint8).tobytes())
        self.routes = None if routes is None else mem.block(4 * max(1, n), (np.asarray(list(routes) or [0], dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).tobytes())
        self.out = mem.block(8 * n)
        self.counts = mem.block(8 * O.KINDS) if with_counts else None
        self.idx = [mem.block(4 * cap) for cap in self.caps]
        self.cnt = [mem.block(4) for _ in self.caps]
        self.batch = _abi.Batch()
        self.batch.struct_size, self.batch.n, self.batch.memory = C.sizeof(_abi.Batch), n, mem.memory
        self.batch.field[2].data, self.batch.field[2].offsets = mem.ptr(self.keep[1]), mem.ptr(self.keep[2])  # PWAF_FIELD_PATH; every other column is NULL
        self.arr = (_abi.RespList * max(1, len(self.masks)))()
        for l, (mask, cap) in enumerate(zip(self.masks, self.caps)):
            self.arr[l].kinds, self.arr[l].cap, self.arr[l].idx, self.arr[l].n = mask, cap, mem.ptr(self.idx[l]) if cap else None, mem.ptr(self.cnt[l])
        self.scratch, self.scratch_bytes = mem.scratch(n)

    def run(self, stream=None, **override):
        """override: batch / verdicts / out / counts / lists / n_lists / scratch / scratch_bytes as the C arguments to pass instead"""
        a = {"batch": C.byref(self.batch), "verdicts": self.mem.ptr(self.keep[0]), "status": None if self.statuses is None else self.mem.ptr(self.statuses),
             "route": None if self.routes is None else self.mem.ptr(self.routes), "out": self.mem.ptr(self.out), "counts": None if self.counts is None else self.mem.ptr(self.counts),
             "lists": self.arr, "n_lists": len(self.masks), "scratch": None if self.scratch is None else self.mem.ptr(self.scratch), "scratch_bytes": self.scratch_bytes}
        a.update(override)
        return lib().pwaf_respond(a["batch"], a["verdicts"], a["status"], a["route"], a["out"], a["counts"], a["lists"], a["n_lists"], a["scratch"], a["scratch_bytes"],
                                  None if stream is None else C.c_void_p(stream))

    def untouched(self):
        """nothing the call may write was written (a refusal)"""
        blocks = [self.out] + ([self.counts] if self.counts is not None else []) + self.idx + self.cnt
        return all((self.mem.read(b) == FILL).all() for b in blocks)

    def results(self, label=""):
        """(responses [(kind, arg)], counts, [(entries written, n)]) after the call has run; asserts every guard and every unwritten entry"""
        n = self.n
        out = self.mem.read(self.out)
        assert (out[8 * n:] == FILL).all(), f"{label}: bytes behind the responses were written"
        rec = out[:8 * n].view(np.uint32).reshape(n, 2)
        assert ((rec[:, 0] >> 8) == 0).all(), f"{label}: a response's pad bytes are not 0"
        resp = [(int(k), int(a)) for k, a in rec]
        counts = None
        if self.counts is not None:
            c = self.mem.read(self.counts)
            assert (c[8 * O.KINDS:] == FILL).all(), f"{label}: bytes behind the counts were written"
            counts = [int(x) for x in c[:8 * O.KINDS].view(np.uint64)]
        lists = []
        for l, cap in enumerate(self.caps):
            cnt = self.mem.read(self.cnt[l])
            assert (cnt[4:] == FILL).all(), f"{label}: bytes behind list {l}'s n were written"
            m = int(cnt[:4].view(np.uint32)[0])
            idx = self.mem.read(self.idx[l])
            written = min(m, cap)
            assert (idx[4 * written:] == FILL).all(), f"{label}: list {l} has {m} members and room for {cap}, and an entry at or past {written} was written"
            lists.append(([int(x) for x in idx[:4 * written].view(np.uint32)], m))
        return resp, counts, lists


def check(label, mem, verdicts, statuses, routes, paths, lists=(), caps=None, stream=None, sync=None, **kw):
    """run one call and compare everything it wrote with the oracle's"""
    call = Call(mem, verdicts, statuses, routes, paths, lists, caps, **kw)
    rc = call.run(stream=stream)
    assert rc == _abi.OK, (label, rc, lib().pwaf_last_error())
    if sync is not None:
        sync()
    got = call.results(label)
    kinds = [tuple(k for k in range(O.KINDS) if m >> k & 1) for m in call.masks]
    want = O.expect_batch(verdicts, statuses, routes, paths, kinds, call.caps)
    assert got[0] == want[0], f"{label}: responses differ; first at {next(i for i, (g, w) in enumerate(zip(got[0], want[0])) if g != w)}"
    assert got[1] is None or got[1] == want[1], f"{label}: counts {got[1]} want {want[1]}"
    for l, (g, w) in enumerate(zip(got[2], want[2])):
        assert g[1] == w[1], f"{label}: list {l} (mask {call.masks[l]:#x}, cap {call.caps[l]}): n {g[1]} want {w[1]}"
        assert g[0] == w[0], f"{label}: list {l} (mask {call.masks[l]:#x}, cap {call.caps[l]}): entries differ"
    return got
