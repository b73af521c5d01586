"""Grammar-constrained decoding: ``TokenGrammar``, a deterministic automaton over token ids (or classes of token ids) whose
state decides which tokens a logit row may emit.  include/specdec.h (sd_grammar) has the definition the native loops
implement; ``sampling.utils.apply_grammar`` states it in torch.  The table interface is the boundary: compiling a regex or a
JSON schema over a tokenizer's strings into such tables is the caller's business."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .._lib import SdGrammar, check, lib


def _table(x, name: str) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        if x.is_floating_point() or x.dtype == torch.bool:
            raise ValueError(f"{name}: an integer table is required, not {x.dtype}")
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name}: an integer table is required, not {a.dtype}")
    return a.astype(np.int64)


class TokenGrammar:
    """``next``: (n_states, n_classes) integers, the state after a token of class c in state s, or -1 where the token is not
    allowed; ``start``: the state the first output token is drawn in; ``classes``: (vocab_size,) integers in [0, n_classes),
    a token's class, or None for the identity (n_classes == vocab_size).  ``masks`` - one bit per state and token id, the
    form the kernel reads - is derived from ``next >= 0``, so the two never disagree.  Validated on the host, ValueError:
    ``next`` outside [-1, n_states), ``classes`` outside [0, n_classes) or of another length than the vocabulary, ``start``
    outside [0, n_states), and a state that is reachable from ``start`` and allows no token (its row would be all -inf on a
    valid path; an unreachable dead end is fine).  ``eos_token_id`` is kept for the builders and the callers; the automaton
    treats EOS like any token."""

    def __init__(self, next, start: int, eos_token_id, vocab_size: int, classes=None):
        nxt = _table(next, "next")
        V = int(vocab_size)
        if nxt.ndim != 2 or nxt.shape[0] < 1 or nxt.shape[1] < 1 or V < 1:
            raise ValueError(f"next: a (n_states >= 1, n_classes >= 1) table is required, not shape {tuple(nxt.shape)} (vocabulary {V})")
        S, K = nxt.shape
        if ((nxt < -1) | (nxt >= S)).any():
            s, c = np.argwhere((nxt < -1) | (nxt >= S))[0]
            raise ValueError(f"next: state {int(s)}, class {int(c)}: {int(nxt[s, c])} lies outside [-1, {S})")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 0 <= int(start) < S:
            raise ValueError(f"start: a state in [0, {S}) is required, not {start!r}")
        if classes is None:
            if K != V:
                raise ValueError(f"classes: without a class table next has one column per token id, {V}, not {K}")
            cls = None
        else:
            cls = _table(classes, "classes").reshape(-1)
            if len(cls) != V:
                raise ValueError(f"classes: {len(cls)} entries for a vocabulary of {V}")
            if ((cls < 0) | (cls >= K)).any():
                t = int(np.argwhere((cls < 0) | (cls >= K))[0, 0])
                raise ValueError(f"classes: token {t}: class {int(cls[t])} lies outside [0, {K})")
        self.next, self.classes = nxt.astype(np.int32), None if cls is None else cls.astype(np.int32)
        self.start, self.vocab_size, self.n_states, self.n_classes = int(start), V, S, K
        self.eos_token_id = None if eos_token_id is None else int(eos_token_id)
        allowed = self.next >= 0                                   # (S, K): the classes a state allows
        if cls is not None:
            used = np.zeros(K, dtype=bool)
            used[cls] = True
            allowed_tok = allowed[:, cls]                          # (S, V)
        else:
            used, allowed_tok = np.ones(K, dtype=bool), allowed
        # every state reachable from start (over classes some token has) allows at least one token
        seen, todo = {self.start}, [self.start]
        while todo:
            s = todo.pop()
            if not allowed_tok[s].any():
                raise ValueError(f"next: state {s} is reachable from start {self.start} and allows no token")
            for to in np.unique(self.next[s][allowed[s] & used]).tolist():
                if to not in seen:
                    seen.add(to)
                    todo.append(to)
        W = (V + 31) // 32
        bits = np.zeros((S, W * 32), dtype=bool)
        bits[:, :V] = allowed_tok
        self.masks = np.packbits(bits.reshape(S, W, 32), axis=2, bitorder="little").view("<u4").reshape(S, W).astype(np.uint32)
        self._device = {}

    # ---- the automaton on the host
    def step(self, state: int, token: int) -> int:
        """sd_grammar's step: the next state, or -1 (dead) for a dead state, a token outside [0, V) or a -1 entry."""
        state, token = int(state), int(token)
        if not 0 <= state < self.n_states or not 0 <= token < self.vocab_size:
            return -1
        to = int(self.next[state, token if self.classes is None else int(self.classes[token])])
        return to if 0 <= to < self.n_states else -1

    def state_after(self, tokens, state=None) -> int:
        """The state after the output tokens ``tokens`` (from ``start``, or from ``state``); -1 once a token was not allowed."""
        s = self.start if state is None else int(state)
        for t in (tokens.reshape(-1).tolist() if isinstance(tokens, (torch.Tensor, np.ndarray)) else tokens):
            s = self.step(s, t)
        return s

    def accepts_prefix(self, tokens) -> bool:
        """Whether every token of ``tokens`` was allowed in the state its predecessors lead to."""
        return self.state_after(tokens) >= 0

    def allowed_ids(self, state: int) -> np.ndarray:
        """The token ids state ``state`` allows, ascending."""
        row = self.next[int(state)] >= 0
        return np.flatnonzero(row if self.classes is None else row[self.classes])

    # ---- builders
    @classmethod
    def from_choices(cls, choices, vocab_size: int, eos_token_id: int) -> "TokenGrammar":
        """The output is one of ``choices`` (sequences of token ids) followed by EOS: a trie of the choices.  At the end of a
        choice only EOS is allowed - beside the tokens that continue a longer choice it is a prefix of.  EOS leads to a free
        state in which every id is allowed: the loops keep drafting past an EOS, and those rows must normalise although nobody
        samples from them."""
        V, eos = int(vocab_size), int(eos_token_id)
        if not 0 <= eos < V:
            raise ValueError(f"eos_token_id: {eos_token_id!r} lies outside [0, {V})")
        choices = [[int(t) for t in (c.reshape(-1).tolist() if isinstance(c, (torch.Tensor, np.ndarray)) else c)] for c in choices]
        if not choices:
            raise ValueError("choices: at least one choice is required")
        rows = [{}]                                                # state -> {token: next state}; state 0 is the root
        ends = set()
        for k, c in enumerate(choices):
            if not c:
                raise ValueError(f"choices: choice {k} is empty")
            s = 0
            for t in c:
                if not 0 <= t < V or t == eos:
                    raise ValueError(f"choices: choice {k}: token {t} lies outside [0, {V}) or is EOS ({eos})")
                if t not in rows[s]:
                    rows.append({})
                    rows[s][t] = len(rows) - 1
                s = rows[s][t]
            ends.add(s)
        free = len(rows)
        nxt = np.full((free + 1, V), -1, dtype=np.int64)
        for s, row in enumerate(rows):
            for t, to in row.items():
                nxt[s, t] = to
            if s in ends:
                nxt[s, eos] = free
        nxt[free, :] = free
        return cls(nxt, 0, eos, V)

    # ---- the device form
    def to_device(self, device) -> "DeviceGrammar":
        """The three tables on ``device``, uploaded once per device and shared by any number of streams."""
        key = str(torch.device(device))
        if key not in self._device:
            self._device[key] = DeviceGrammar(self, device)
        return self._device[key]


class DeviceGrammar:
    """A TokenGrammar's tables on one device and the sd_grammar that points at them (which it keeps alive)."""

    def __init__(self, grammar: TokenGrammar, device):
        self.grammar = grammar
        self.masks = torch.from_numpy(grammar.masks.view(np.int32).copy()).to(device)
        self.next = torch.from_numpy(grammar.next.copy()).to(device)
        self.cls = torch.from_numpy(grammar.classes.copy()).to(device) if grammar.classes is not None else None
        self.block = SdGrammar(self.masks.data_ptr(), self.next.data_ptr(), self.cls.data_ptr() if self.cls is not None else None,
                               grammar.n_states, grammar.n_classes, grammar.start)

    def pointer(self):
        return C.pointer(self.block)


GRAMMAR_NEEDS_NATIVE = 'grammar needs the native loop: rng="device" (or a device noise object)'


def grammar_list(n: int, what: str, grammar):
    """``grammar`` of a call with ``n`` streams: None, one TokenGrammar for all, or a sequence with one TokenGrammar-or-None per
    ``what`` -> None when nobody has one, else the n entries.  ValueError for anything else.  Touches no GPU."""
    if grammar is None:
        return None
    if isinstance(grammar, TokenGrammar):
        return [grammar] * n
    if not isinstance(grammar, (list, tuple)):
        raise ValueError(f"grammar: a TokenGrammar, or one TokenGrammar (or None) per {what}, is required, not {grammar!r}")
    if len(grammar) != n:
        raise ValueError(f"grammar: {len(grammar)} entries for {n} {what}s")
    for i, g in enumerate(grammar):
        if g is not None and not isinstance(g, TokenGrammar):
            raise ValueError(f"grammar: {what} {i}: a TokenGrammar or None is required, not {g!r}")
    return list(grammar) if any(g is not None for g in grammar) else None


def grammar_needs_target_rows(target_m) -> None:
    """A grammar masks the logit rows where a single-GPU forward leaves them: a tensor-parallel shard is refused."""
    if getattr(target_m, "tp_group", None) is not None:
        raise ValueError("grammar is not available with a tensor-parallel target model")


def check_grammar_vocab(grammars, what: str, V: int) -> None:
    for i, g in enumerate(grammars or ()):
        if g is not None and g.vocab_size != V:
            raise ValueError(f"grammar: {what} {i}: built for a vocabulary of {g.vocab_size}, the model's is {V}")


class GrammarBinding:
    """The grammars of one native loop call attached to the streams' target sessions: per session with a grammar a device
    state cache of ``caps[i]`` ints (states[j] = the state output token j is drawn in) and sd_session_set_grammar.  ``detach()``
    (always, also after a failure) takes them off again: a session outlives the call."""

    def __init__(self, sessions, grammars, caps, device):
        self._sessions = []
        self.states = []
        try:
            for ses, g, cap in zip(sessions, grammars, caps):
                if g is None:
                    self.states.append(None)
                    continue
                st = torch.full((max(1, int(cap)),), -1, dtype=torch.int32, device=device)
                self.states.append(st)
                check(lib.sd_session_set_grammar(ses.handle, g.to_device(device).pointer(), st.data_ptr(), st.numel()),
                      "sd_session_set_grammar")
                self._sessions.append(ses)
        except Exception:
            self.detach()
            raise

    def detach(self) -> None:
        for ses in self._sessions:
            lib.sd_session_set_grammar(ses.handle, None, None, 0)
        self._sessions = []
