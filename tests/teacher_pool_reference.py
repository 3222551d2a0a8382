"""A numpy restatement of the teacher's stream pool (include/gitcap.h: gitcap_pool_*): the host plan that maps per-stream ring
cursors to the tables of a push and of a pool call (csrc/host_logic.h: pool_plan), and what the two kernels do with them
(csrc/rowops.hip: pool_scatter_kernel, pool_assemble_kernel).  Written from the header's description alone, stream by stream and
frame by frame, with none of the library's modular arithmetic; GPU_* are the inputs the CPU and the GPU tests share."""
import numpy as np


class Refused(Exception):
    """A plan the library refuses; .state: with GITCAP_ERR_STATE (a named stream holds nothing) rather than GITCAP_ERR_ARG."""

    def __init__(self, why, state=False):
        super().__init__(why)
        self.state = state


class Pool:
    """S streams of F slots as explicit lists: order[s] = the slots of the frames stream s holds, oldest first, and nxt[s] = the
    slot its next frame goes to."""

    def __init__(self, S, F):
        self.S, self.F = S, F
        self.order = [[] for _ in range(S)]
        self.nxt = [0] * S

    def heads(self):
        return list(self.nxt)

    def counts(self):
        return [len(o) for o in self.order]

    def push(self, ids):
        """-> dst [n]: the ring frame (stream * F + slot) of every pushed frame; the streams advance."""
        per = {}
        for s in ids:
            if not 0 <= s < self.S:
                raise Refused(f"stream {s} out of range")
            per[s] = per.get(s, 0) + 1
            if per[s] > self.F:
                raise Refused(f"more than F frames for stream {s}")
        dst = []
        for s in ids:
            k = self.nxt[s]
            if k in self.order[s]:                  # the slot of the oldest frame: it leaves
                self.order[s].remove(k)
            self.order[s].append(k)
            self.nxt[s] = k + 1 if k + 1 < self.F else 0
            dst.append(s * self.F + k)
        return dst

    def call(self, ids):
        """-> src, pos [packed frames], off, len [B], (total, longest, dense) of a pool call on streams `ids`"""
        if not ids:
            raise Refused("no stream named")
        for r, s in enumerate(ids):
            if not 0 <= s < self.S:
                raise Refused(f"stream {s} out of range")
            if s in ids[:r]:
                raise Refused(f"stream {s} twice")
        for s in ids:
            if not self.order[s]:
                raise Refused(f"stream {s} holds nothing", state=True)
        src, pos, off, ln = [], [], [], []
        for s in ids:
            off.append(len(src))
            ln.append(len(self.order[s]))
            for f, k in enumerate(self.order[s]):
                src.append(s * self.F + k)
                pos.append(f)
        return src, pos, off, ln, (len(src), max(ln), int(len(set(ln)) == 1))


def scatter(ring, stage, dst):
    """ring [ring_frames][N][D] (changed in place and returned) <- stage [n][N][D]: frame i to ring frame dst[i]"""
    for i, d in enumerate(dst):
        ring[d] = stage[i]
    return ring


def assemble(ring, temporal, src, pos):
    """-> the fp32 sums [len(src) * N][D]: packed frame g = ring[src[g]] + temporal[pos[g]] (temporal None: no add)"""
    out = np.stack([ring[s].astype(np.float32) + (0 if temporal is None else temporal[p].astype(np.float32)[None, :])
                    for s, p in zip(src, pos)]).astype(np.float32)
    return out.reshape(-1, ring.shape[-1])


def bf16_round(x):
    """fp32 -> the bf16 bit patterns (uint16), round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


# What the GPU kernel tests run: three streams of F = 3; stream 1 was pushed to five times (wrapped, its next slot is the last),
# stream 0 once, stream 2 never; then a push of 5 frames in mixed order that takes stream 1 across the wrap again and gives stream 2 two frames.
GPU_S, GPU_F = 3, 3
GPU_HISTORY = [[1, 0], [1], [1], [1], [1]]
GPU_PUSH = [2, 1, 0, 2, 1]


def gpu_pool():
    p = Pool(GPU_S, GPU_F)
    for ids in GPU_HISTORY:
        p.push(ids)
    return p
