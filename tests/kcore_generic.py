"""The k-core decomposition as a generic vertex program without a combiner: the H-index iteration
over every vertex's whole message list (tgo_gather_lists).  tests/test_gpu_kcore.py compares it
with tgo_kcore bit for bit, scripts/kcore_bench.py times it as the baseline the native program
replaces.  It needs a duplicate-free, loop-free edge list: a vertex's first message count is its
degree."""
import numpy as np

from titan_amd import GenericVertexProgram, MessageScope
from titan_amd import _lib as L


def simple_edges(n, src, dst):
    """The edge list with loops dropped and every unordered pair kept once."""
    src, dst = np.asarray(src), np.asarray(dst)
    keep = src != dst
    lo = np.minimum(src[keep], dst[keep]).astype(np.int64)
    hi = np.maximum(src[keep], dst[keep]).astype(np.int64)
    key = np.unique(lo * n + hi)
    return (key // n).astype(np.int32), (key % n).astype(np.int32)


class GenericKCore(GenericVertexProgram):
    """Every vertex keeps c = min(c, H-index of its neighbours' c), starting from its number of
    messages, until a superstep changes nothing."""
    value_type = L.VAL_INT64
    combiner = None
    compute_keys = ("core",)
    memory_compute_keys = ("changes",)
    SCOPE = MessageScope.Local("bothE")

    def __init__(self):
        self._last = -1

    def getMessageScopes(self, memory):  # noqa: N802
        return [self.SCOPE]

    def execute(self, v, messenger, memory):
        if memory.isInitialIteration():
            messenger.send(self.SCOPE, np.zeros(v.n, np.int64))
            memory.incr("changes", 0)
            return
        lists = messenger.receive(self.SCOPE)
        cnt = lists.counts()
        if memory.getIteration() == 1:
            new = cnt.astype(np.int64)
            changed = v.n
        else:
            cur, _ = v.property("core")
            rows = np.repeat(np.arange(v.n), cnt)
            order = np.lexsort((-lists.values, rows))       # each vertex's messages, largest first
            rank = np.arange(len(rows)) - lists.offsets[:-1][rows] + 1
            h = np.bincount(rows, weights=(lists.values[order] >= rank), minlength=v.n).astype(np.int64)
            new = np.minimum(cur, h)
            changed = int((new != cur).sum())
        v.set_property("core", new)
        messenger.send(self.SCOPE, new)
        memory.incr("changes", changed)

    def terminate(self, memory):
        total = memory.get("changes")
        done = memory.getIteration() > 1 and total == self._last
        self._last = total
        return done
