"""Peer-pressure clustering as a generic vertex program without a combiner: what a user had to write
before tgo_peer_pressure (tests/test_gpu_peer_pressure.py compares it with the native program bit for
bit, scripts/pp_bench.py times it as the baseline the native program replaces).

A vertex's message is one int64, rank << 33 | S: the rank of its cluster's Titan id and its vote
strength in units of 2^-32.  Superstep 0 sends a word along the reverse of the vote scope, so that in
superstep 1 the length of a vertex's list is d(v), the entries it sends over.  From then on every
superstep is one voting round: tgo_gather_lists hands every vertex's whole message list to the host,
where the lists are grouped by (vertex, rank), summed exactly in uint64 and the largest tally taken,
ties to the smallest rank."""
import numpy as np

from titan_amd import GenericVertexProgram, MessageScope
from titan_amd import _lib as L

REVERSE = {"outE": "inE", "inE": "outE", "bothE": "bothE"}
MASK = np.uint64((1 << 33) - 1)
ONE = 1 << 32


class GenericPeerPressure(GenericVertexProgram):
    value_type = L.VAL_INT64
    combiner = None
    compute_keys = ("cluster",)

    def __init__(self, edges="outE", distribute=False, max_rounds=30):
        self.vote = MessageScope.Local(edges)
        self.back = MessageScope.Local(REVERSE[edges])
        self.distribute = bool(distribute)
        self.max_rounds = int(max_rounds)
        self.rounds = 0
        self.changed = -1
        self.done = False

    def getMessageScopes(self, memory):  # noqa: N802
        return [self.vote, self.back]

    def _words(self):
        return ((self.rank.astype(np.uint64) << np.uint64(33)) | self.strength).view(np.int64)

    def _finish(self, v):
        v.set_property("cluster", self.sorted_ids[self.rank])
        self.done = True

    def execute(self, v, messenger, memory):
        if memory.isInitialIteration():
            order = np.argsort(v.ids, kind="stable")
            self.sorted_ids = np.asarray(v.ids, np.int64)[order]
            self.rank = np.empty(v.n, np.int64)
            self.rank[order] = np.arange(v.n)
            messenger.send(self.back, np.zeros(v.n, np.int64))
            return
        if memory.getIteration() == 1:
            d = messenger.receive(self.back).counts()
            self.sends = d > 0
            self.strength = np.full(v.n, ONE, np.uint64)
            if self.distribute:
                self.strength = np.where(self.sends, ONE // np.maximum(d, 1), 0).astype(np.uint64)
            if self.max_rounds == 0 or v.n == 0:
                return self._finish(v)
            messenger.send(self.vote, self._words())
            return
        lists = messenger.receive(self.vote)
        words = lists.values[:lists.offsets[-1]].view(np.uint64)
        owner = np.concatenate([np.repeat(np.arange(v.n, dtype=np.int64), lists.counts()), np.arange(v.n, dtype=np.int64)])
        label = np.concatenate([(words >> np.uint64(33)).astype(np.int64), self.rank])
        s = np.concatenate([words & MASK, self.strength])
        order = np.lexsort((label, owner))
        owner, label, s = owner[order], label[order], s[order]
        head = np.flatnonzero(np.r_[True, (owner[1:] != owner[:-1]) | (label[1:] != label[:-1])])
        tally = np.add.reduceat(s, head)                        # exact: uint64
        g_owner, g_label = owner[head], label[head]
        first = np.flatnonzero(np.r_[True, g_owner[1:] != g_owner[:-1]])    # every vertex has its own vote
        most = np.maximum.reduceat(tally, first)
        hit = np.flatnonzero(tally == most[g_owner])            # groups are in rank order: the first hit wins
        _, pick = np.unique(g_owner[hit], return_index=True)
        new = g_label[hit[pick]]
        if self.distribute:
            new = np.where(self.sends, new, self.rank)          # d(v) = 0: the vertex never leaves
        self.changed = int((new != self.rank).sum())
        self.rank = new
        self.rounds += 1
        if self.changed == 0 or self.rounds == self.max_rounds:
            return self._finish(v)
        messenger.send(self.vote, self._words())

    def terminate(self, memory):
        return self.done
