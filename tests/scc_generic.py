"""Strongly connected components as a generic vertex program: the colouring of tgo_scc run
superstep by superstep (tests/test_gpu_scc.py compares it with the native program bit for bit,
scripts/scc_bench.py times it as the baseline the native program replaces).

A pass: every live vertex starts with its own Titan id as its colour; the colours travel forward
along the arcs under a MAX combiner (MessageScope.Local("outE")) until a superstep changes none; the
vertices that kept their own colour are roots and are marked; the marked vertices send their colour
backward (MessageScope.Local("inE")) under a MIN combiner — every colour a vertex hears from the
head of one of its arcs is at least its own, so the minimum equals its colour exactly when a marked
vertex of its colour is among them — and an unmarked vertex that hears its own colour is marked; when
a superstep marks none, the marked vertices retire under their colour.  Passes repeat while a
vertex is live.  The label is the smallest Titan id of the component."""
import numpy as np

from titan_amd import GenericVertexProgram, MessageScope
from titan_amd import _lib as L


class GenericScc(GenericVertexProgram):
    value_type = L.VAL_INT64
    combiner = L.COMBINE_MAX            # switched to MIN for the backward supersteps
    compute_keys = ("scc",)
    memory_compute_keys = ("passes",)
    FORWARD = MessageScope.Local("outE")
    BACKWARD = MessageScope.Local("inE")

    def __init__(self):
        self.done = False
        self.passes = 0

    def getMessageScopes(self, memory):  # noqa: N802
        return [self.FORWARD, self.BACKWARD]

    def _start_pass(self, v, messenger):
        self.passes += 1
        self.colour = np.where(self.live, v.ids, 0).astype(np.int64)
        self.mark = np.zeros(v.n, bool)
        self.forward = True
        messenger.send(self.FORWARD, self.colour, self.live)

    def execute(self, v, messenger, memory):
        if memory.isInitialIteration():
            self.live = np.ones(v.n, bool)
            self.rep = np.zeros(v.n, np.int64)
            memory.incr("passes", 0)
            self._start_pass(v, messenger)
            return
        if self.forward:
            self.combiner = L.COMBINE_MAX
            got, has = messenger.receive(self.FORWARD)
            better = self.live & has & (got > self.colour)
            self.colour[better] = got[better]
            if better.any():
                messenger.send(self.FORWARD, self.colour, self.live)
                return
            self.forward = False
            self.mark = self.live & (self.colour == v.ids)
            messenger.send(self.BACKWARD, self.colour, self.mark)
            return
        self.combiner = L.COMBINE_MIN
        got, has = messenger.receive(self.BACKWARD)
        new = self.live & ~self.mark & has & (got == self.colour)
        self.mark |= new
        if new.any():
            messenger.send(self.BACKWARD, self.colour, self.mark)
            return
        self.rep[self.mark] = self.colour[self.mark]
        self.live &= ~self.mark
        memory.incr("passes", 1)
        if self.live.any():
            self._start_pass(v, messenger)
            return
        _, inv = np.unique(self.rep, return_inverse=True)
        lo = np.full(inv.max() + 1 if v.n else 0, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(lo, inv, v.ids)
        v.set_property("scc", lo[inv])
        self.done = True

    def terminate(self, memory):
        return self.done
