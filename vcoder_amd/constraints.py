"""Constrained decoding: a deterministic automaton over token ids that generate(constraint=) applies inside the device decode loop
(csrc/select.hip logits_process_kernel, phase 4; vc_request_constraint) and, through `as_prefix_allowed_tokens_fn`, on the host
loops — HF 4.31's `prefix_allowed_tokens_fn` / PrefixConstrainedLogitsProcessor.  The callable IS the definition: the device loop
must return what the host loop returns under it.

Tables (CSR, int32): state s owns the edges state_off[s] .. state_off[s + 1]; edge_tok is ascending and unique within a state,
edge_next the state behind the edge.  default_next[s] >= 0: s is a free-text state — every token without an edge is allowed too and
leads there; -1: only the tokens with an edge are allowed.  State 0 is the start; state -1 is dead (nothing is allowed).  A token
that has an edge is allowed whatever the edge leads to."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

MAX_STATES = 65536       # what vc_request_constraint accepts (include/vcoder_hip.h)
MAX_EDGES = 1 << 20
DEAD = -1


def _ids(name, seq, allow_empty=False) -> List[int]:
    if isinstance(seq, (str, bytes)) or not hasattr(seq, "__iter__"):
        raise ValueError(f"`{name}` has to be a list of token ids, but is {seq!r}")
    out = []
    for t in seq:
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or int(t) < 0:
            raise ValueError(f"`{name}` has to hold non-negative token ids, but holds {t!r}")
        out.append(int(t))
    if not out and not allow_empty:
        raise ValueError(f"`{name}` must not be empty")
    return out


class TokenAutomaton:
    def __init__(self, state_off, edge_tok, edge_next, default_next, final=()):
        self.state_off, self.edge_tok, self.edge_next, self.default_next = state_off, edge_tok, edge_next, default_next
        self.final = frozenset(int(s) for s in final)   # states behind a complete answer (the builders'; informational)

    # ---- builders ------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_edges(cls, state_off, edge_tok, edge_next, default_next, final=()) -> "TokenAutomaton":
        """raw tables -> a validated automaton (ValueError otherwise)"""
        def arr(name, a):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
                raise ValueError(f"`{name}` has to be a 1-D integer array")
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError(f"`{name}` does not fit int32")
            return np.ascontiguousarray(a, dtype=np.int32)

        off, tok, nxt, dflt = arr("state_off", state_off), arr("edge_tok", edge_tok), arr("edge_next", edge_next), arr("default_next", default_next)
        S, E = dflt.size, tok.size
        if S < 1 or S > MAX_STATES:
            raise ValueError(f"an automaton has 1 .. {MAX_STATES} states, got {S}")
        if E > MAX_EDGES:
            raise ValueError(f"an automaton has at most {MAX_EDGES} edges, got {E}")
        if off.size != S + 1 or nxt.size != E or off[0] != 0 or off[-1] != E or (np.diff(off) < 0).any():
            raise ValueError("state_off has to rise from 0 to the number of edges over S + 1 entries, edge_next to match edge_tok")
        for name, a in (("edge_next", nxt), ("default_next", dflt)):
            if a.size and (a.min() < DEAD or a.max() >= S):
                raise ValueError(f"`{name}` holds a target outside [-1, {S})")
        if E > 1:
            inner = np.ones(E - 1, dtype=bool)
            inner[off[1:-1][(off[1:-1] > 0) & (off[1:-1] < E)] - 1] = False   # pairs that straddle two states
            bad = np.nonzero(inner & (np.diff(tok.astype(np.int64)) <= 0))[0]
            if bad.size:
                s = int(np.searchsorted(off, bad[0], side="right") - 1)
                raise ValueError(f"state {s}: edge tokens have to be ascending and unique (ids {int(tok[bad[0]])}, {int(tok[bad[0] + 1])})")
        reach = np.zeros(S, dtype=bool)
        reach[0] = True
        front = np.asarray([0])
        while front.size:
            t = np.concatenate([nxt[off[s]:off[s + 1]] for s in front] + [dflt[front]])
            t = np.unique(t[t >= 0])
            front = t[~reach[t]]
            reach[front] = True
        stuck = np.nonzero(reach & (dflt < 0) & (np.diff(off) == 0))[0]
        if stuck.size:
            raise ValueError(f"state {int(stuck[0])} is reachable and allows no token")
        return cls(off, tok, nxt, dflt, final)

    @classmethod
    def _from_dicts(cls, edges: List[Dict[int, int]], final) -> "TokenAutomaton":
        off, tok, nxt = [0], [], []
        for e in edges:
            for t in sorted(e):
                tok.append(t)
                nxt.append(e[t])
            off.append(len(tok))
        return cls.from_edges(np.asarray(off, dtype=np.int64), np.asarray(tok, dtype=np.int64), np.asarray(nxt, dtype=np.int64),
                              np.full(len(edges), DEAD, dtype=np.int64), final)

    @staticmethod
    def _end(edges, end_ids) -> int:
        """the state behind a complete answer: only the end ids, for ever (a row past its end id is finished when the end id is the
        call's EOS; otherwise it keeps emitting end ids)"""
        edges.append({})
        f = len(edges) - 1
        for e in end_ids:
            edges[f][e] = f
        return f

    @classmethod
    def from_sequences(cls, seqs: Sequence[Sequence[int]], end_ids: Sequence[int]) -> "TokenAutomaton":
        """the answer is exactly one of `seqs` (id lists), then one of `end_ids`"""
        end_ids = _ids("end_ids", end_ids)
        seqs = [_ids("seqs[..]", q) for q in seqs]
        if not seqs:
            raise ValueError("`seqs` must not be empty")
        edges: List[Dict[int, int]] = [{}]
        ends = []
        for q in seqs:
            s = 0
            for t in q:
                if t not in edges[s]:
                    edges.append({})
                    edges[s][t] = len(edges) - 1
                s = edges[s][t]
            ends.append(s)
        f = cls._end(edges, end_ids)
        for s in sorted(set(ends)):
            clash = sorted(set(end_ids) & set(edges[s]))
            if clash:
                raise ValueError(f"nondeterministic: end ids {clash} also continue a longer sequence")
            for e in end_ids:
                edges[s][e] = f
        return cls._from_dicts(edges, [f])

    @classmethod
    def from_list(cls, prefix: Sequence[int], items: Sequence[Sequence[int]], separator: Sequence[int], terminator: Sequence[int],
                  end_ids: Sequence[int], min_items: int = 1, max_items: Optional[int] = None) -> "TokenAutomaton":
        """prefix item (separator item)* terminator end, with min_items .. max_items items (None: no upper bound).  All arguments are
        id lists; prefix and terminator may be empty.  The items form a trie whose item-end states carry the separator and terminator
        edges; a separator / terminator (/ end, behind an empty terminator) first id that also continues a longer item there makes the
        answer nondeterministic: ValueError naming the ids."""
        prefix, terminator = _ids("prefix", prefix, True), _ids("terminator", terminator, True)
        separator, end_ids = _ids("separator", separator), _ids("end_ids", end_ids)
        items = [_ids("items[..]", q) for q in items]
        if not items:
            raise ValueError("`items` must not be empty")
        if isinstance(min_items, bool) or not isinstance(min_items, int) or min_items < 1:
            raise ValueError(f"`min_items` has to be a positive integer, but is {min_items!r}")
        if max_items is not None and (isinstance(max_items, bool) or not isinstance(max_items, int) or max_items < min_items):
            raise ValueError(f"`max_items` has to be an integer >= min_items or None, but is {max_items!r}")
        layers = max_items if max_items is not None else min_items
        edges: List[Dict[int, int]] = [{}]

        def new():
            edges.append({})
            return len(edges) - 1

        s = 0
        for t in prefix:
            edges[s][t] = new()
            s = edges[s][t]
        roots = [s] + [new() for _ in range(layers - 1)]
        # the terminator's tail and the end state are shared by every item end; so is a layer's separator tail
        f = cls._end(edges, end_ids)
        close = terminator if terminator else None
        term_in = f
        if terminator:
            for t in reversed(terminator[1:] + [None]):   # states behind terminator[0], [1], ..: the last one carries the end ids
                st = new()
                if t is None:
                    for e in end_ids:
                        edges[st][e] = f
                else:
                    edges[st][t] = term_in
                term_in = st
        for j, root in enumerate(roots):
            done = j + 1                                    # items complete at this layer's item ends
            more = max_items is None or done < max_items
            nxt_root = roots[min(j + 1, layers - 1)]
            sep_in = nxt_root
            for t in reversed(separator[1:]):
                st = new()
                edges[st][t] = sep_in
                sep_in = st
            ends = []
            for q in items:
                s = root
                for t in q:
                    if t not in edges[s]:
                        edges[s][t] = new()
                    s = edges[s][t]
                ends.append(s)
            for s in sorted(set(ends)):
                out = {}
                if more:
                    out[separator[0]] = sep_in
                if done >= min_items:
                    firsts = [close[0]] if close else end_ids
                    for t in firsts:
                        if t in out:
                            raise ValueError(f"nondeterministic: id {t} starts both the separator and the terminator")
                        out[t] = term_in
                clash = sorted(set(out) & set(edges[s]))
                if clash:
                    raise ValueError(f"nondeterministic: ids {clash} continue a longer item and start the separator / terminator")
                edges[s].update(out)
        return cls._from_dicts(edges, [f])

    # ---- pure-Python semantics -------------------------------------------------------------------------------------------------
    @property
    def num_states(self) -> int:
        return int(self.default_next.size)

    @property
    def num_edges(self) -> int:
        return int(self.edge_tok.size)

    def tables(self):
        return self.state_off, self.edge_tok, self.edge_next, self.default_next

    def allowed(self, state: int, vocab_size: Optional[int] = None) -> List[int]:
        """ids allowed in `state` (those below vocab_size, when given).  A free-text state needs vocab_size."""
        if state < 0 or state >= self.num_states:
            return []
        if self.default_next[state] >= 0:
            if vocab_size is None:
                raise ValueError(f"state {state} allows every token: pass vocab_size")
            return list(range(int(vocab_size)))
        t = self.edge_tok[self.state_off[state]:self.state_off[state + 1]]
        if vocab_size is not None:
            t = t[(t >= 0) & (t < vocab_size)]
        return [int(x) for x in t]

    def step(self, state: int, token: int) -> int:
        if state < 0 or state >= self.num_states:
            return DEAD
        lo, hi = int(self.state_off[state]), int(self.state_off[state + 1])
        k = lo + int(np.searchsorted(self.edge_tok[lo:hi], token))
        if k < hi and int(self.edge_tok[k]) == int(token):
            return int(self.edge_next[k])
        return int(self.default_next[state])

    def walk(self, ids, state: int = 0) -> int:
        """the state behind `ids` from `state`; -1 (dead) once a token was not allowed"""
        for t in ids:
            state = self.step(state, int(t))
            if state < 0:
                return DEAD
        return state

    def as_prefix_allowed_tokens_fn(self, prompt_len: int, vocab_size: Optional[int] = None):
        """HF's callable fn(batch_id, input_ids) -> allowed ids: walks input_ids[prompt_len:] from state 0"""
        def fn(batch_id, input_ids):
            gen = input_ids[prompt_len:]
            return self.allowed(self.walk(gen.tolist() if hasattr(gen, "tolist") else gen), vocab_size)
        return fn
