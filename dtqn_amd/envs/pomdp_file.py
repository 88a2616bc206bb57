"""Tabular POMDPs from Cassandra `.pomdp` files: `load_pomdp(path_or_text) -> PomdpModel`, pure Python and numpy.

Preamble: `discount:`, `values: reward|cost` (cost negates R), `states:` / `actions:` / `observations:` as a count or a name list,
`start:` as a probability row, `uniform` or one state, `start include:` / `start exclude:` (default: uniform).

Entries, every standard form -- names or indices, `*` in every position, later entries override earlier ones, `#` comments:
    T: a : s : s' p        T: a : s <row | uniform>        T: a <matrix | uniform | identity>
    O: a : s' : z p        O: a : s' <row | uniform>       O: a <matrix | uniform>
    R: a : s : s' : z v    R: a : s : s' <row>             R: a : s <matrix>
Episodic extension: `T: a : s reset` marks the pair (s, a) as ending the episode; its T row becomes the start distribution.

The CDFs every draw uses, on the host and on the device, are derived here, once: cdf = cumsum(p) in float64 with every entry from the
last positive probability onward set to exactly 1.0.  The draw rule everywhere is "the first k with u < cdf[k]", which is
np.searchsorted(cdf, u, side="right"): no u in [0, 1) falls through and a zero-probability entry is never drawn.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

MAX_TABLE_BYTES = 256 << 20      # dense start + T + O + R + D
MAX_ACTIONS = 255                # actions are u8 in the replay
MAX_OBSERVATIONS = 65535
ROW_SUM_TOLERANCE = 1e-6

_HEAD = re.compile(r"^\s*(discount|values|states|actions|observations|start\s+include|start\s+exclude|start|T|O|R)\s*:(.*)$")


def cdf_rows(p: np.ndarray) -> np.ndarray:
    """CDF of every row (last axis) of `p`: the float64 cumulative sum, capped at 1.0, with every entry from the row's last positive
    probability onward set to exactly 1.0."""
    p = np.asarray(p, dtype=np.float64)
    cdf = np.minimum(np.cumsum(p, axis=-1, dtype=np.float64), 1.0)
    n = p.shape[-1]
    last = n - 1 - np.argmax((p > 0)[..., ::-1], axis=-1)            # index of the last positive entry of every row
    cdf[np.arange(n) >= last[..., None]] = 1.0
    return cdf


def draw(cdf: np.ndarray, u: float) -> int:
    """The first k with u < cdf[k], clamped to the row."""
    return min(int(np.searchsorted(cdf, u, side="right")), len(cdf) - 1)


@dataclass
class PomdpModel:
    discount: float
    state_names: List[str]
    action_names: List[str]
    observation_names: List[str]
    start: np.ndarray            # [S]
    T: np.ndarray                # [A][S][S']
    O: np.ndarray                # [A][S'][Z]
    R: np.ndarray                # [A][S][S'][Z]
    D: np.ndarray                # [A][S] bool: the pair ends the episode
    episodic: bool
    start_cdf: np.ndarray
    T_cdf: np.ndarray
    O_cdf: np.ndarray

    @property
    def sizes(self) -> Tuple[int, int, int]:
        """(S, A, Z)."""
        return len(self.state_names), len(self.action_names), len(self.observation_names)

    def pack(self, offsets: Sequence[int], nbytes: int) -> np.ndarray:
        """The device's table buffer: start_cdf | T_cdf | O_cdf | R | D (u8) at the given byte offsets (dtqn_pomdp_table_bytes)."""
        buf = np.zeros(int(nbytes), dtype=np.uint8)
        for off, arr in zip(offsets, (self.start_cdf, self.T_cdf, self.O_cdf, self.R, self.D.astype(np.uint8))):
            raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
            buf[int(off):int(off) + raw.size] = raw
        return buf


def table_bytes(S: int, A: int, Z: int) -> int:
    return 8 * (S + A * S * S + A * S * Z + A * S * S * Z) + A * S


class _Parser:
    def __init__(self, text: str):
        self.statements = []                 # (keyword, header line, header rest, [(token, line)] of the continuation lines)
        for no, raw in enumerate(text.splitlines(), 1):
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            m = _HEAD.match(line)
            if m:
                self.statements.append((re.sub(r"\s+", " ", m.group(1)), no, m.group(2), []))
            elif self.statements:
                self.statements[-1][3].extend((tok, no) for tok in line.split())
            else:
                raise ValueError(f"line {no}: expected a preamble keyword, found {line!r}")
        self.last_line = max((s[3][-1][1] if s[3] else s[1]) for s in self.statements) if self.statements else 0

    # ---- helpers ------------------------------------------------------------------------------
    @staticmethod
    def _number(tok: str, line: int) -> float:
        try:
            return float(tok)
        except ValueError:
            raise ValueError(f"line {line}: expected a number, found {tok!r}") from None

    def _prob(self, tok: str, line: int) -> float:
        v = self._number(tok, line)
        if v < 0:
            raise ValueError(f"line {line}: negative probability {tok}")
        return v

    @staticmethod
    def _index(tok: str, names: List[str], what: str, line: int):
        """A name or an index -> slice(None) for `*`, else the index."""
        if tok == "*":
            return slice(None)
        if tok in names:
            return names.index(tok)
        if re.fullmatch(r"\d+", tok):
            k = int(tok)
            if k >= len(names):
                raise ValueError(f"line {line}: {what} index {k} out of range (there are {len(names)})")
            return k
        raise ValueError(f"line {line}: unknown {what} {tok!r}")

    @staticmethod
    def _names(rest: str, toks, what: str, line: int) -> List[str]:
        words = rest.split() + [t for t, _ in toks]
        if not words:
            raise ValueError(f"line {line}: `{what}:` needs a count or a list of names")
        if len(words) == 1 and re.fullmatch(r"\d+", words[0]):
            if int(words[0]) < 1:
                raise ValueError(f"line {line}: `{what}:` needs at least one entry")
            return [str(k) for k in range(int(words[0]))]
        if len(set(words)) != len(words):
            raise ValueError(f"line {line}: `{what}:` repeats a name")
        return words

    # ---- the model ------------------------------------------------------------------------------
    def parse(self) -> PomdpModel:
        discount, sign = 1.0, 1.0
        names = {}
        start_stmt = None
        entries = []
        for kw, line, rest, toks in self.statements:
            if kw == "discount":
                discount = self._number((rest.split() + [t for t, _ in toks] + [""])[0], line)
            elif kw == "values":
                word = (rest.split() + [t for t, _ in toks] + [""])[0]
                if word not in ("reward", "cost"):
                    raise ValueError(f"line {line}: `values:` is `reward` or `cost`, not {word!r}")
                sign = -1.0 if word == "cost" else 1.0
            elif kw in ("states", "actions", "observations"):
                names[kw] = self._names(rest, toks, kw, line)
            elif kw.startswith("start"):
                start_stmt = (kw, line, rest, toks)
            else:
                entries.append((kw, line, rest, toks))
        for kw in ("states", "actions", "observations"):
            if kw not in names:
                raise ValueError(f"line {self.last_line}: the preamble has no `{kw}:`")
        sn, an, zn = names["states"], names["actions"], names["observations"]
        S, A, Z = len(sn), len(an), len(zn)
        if A > MAX_ACTIONS:
            raise ValueError(f"{A} actions exceed the limit of {MAX_ACTIONS} (actions are u8 in the replay)")
        if Z > MAX_OBSERVATIONS:
            raise ValueError(f"{Z} observations exceed the limit of {MAX_OBSERVATIONS}")
        if table_bytes(S, A, Z) > MAX_TABLE_BYTES:
            raise ValueError(f"dense tables of {table_bytes(S, A, Z)} bytes exceed the limit of 256 MiB ({MAX_TABLE_BYTES} bytes)")
        start, start_line = self._start(start_stmt, sn)
        T, O, R = np.zeros((A, S, S)), np.zeros((A, S, Z)), np.zeros((A, S, S, Z))
        D = np.zeros((A, S), dtype=bool)
        t_line, o_line = np.full((A, S), self.last_line), np.full((A, S), self.last_line)
        for kw, line, rest, toks in entries:
            fields = [f.split() for f in rest.split(":")]
            if any(len(f) == 0 for f in fields) or any(len(f) > 1 for f in fields[:-1]):
                raise ValueError(f"line {line}: malformed `{kw}:` entry")
            idx = [f[0] for f in fields]
            vals = [(t, line) for t in fields[-1][1:]] + list(toks)
            if kw == "T":
                self._entry_T(idx, vals, line, T, D, t_line, sn, an)
            elif kw == "O":
                self._entry_O(idx, vals, line, O, o_line, sn, an, zn)
            else:
                self._entry_R(idx, vals, line, R, sn, an, zn)
        T[D] = start                                              # a reset pair: the next state is a fresh start
        self._check_rows(start[None, None], np.full((1, 1), start_line), "start")
        self._check_rows(T, t_line, "T")
        self._check_rows(O, o_line, "O")
        return PomdpModel(discount=discount, state_names=sn, action_names=an, observation_names=zn, start=start, T=T, O=O, R=R if sign > 0 else 0.0 - R,
                          D=D, episodic=bool(D.any()), start_cdf=cdf_rows(start), T_cdf=cdf_rows(T), O_cdf=cdf_rows(O))

    @staticmethod
    def _check_rows(table, lines, what):
        sums = table.sum(axis=-1)
        bad = np.argwhere(np.abs(sums - 1.0) > ROW_SUM_TOLERANCE)
        if len(bad):
            k = tuple(bad[0])
            raise ValueError(f"line {int(lines[k])}: the {what} row {list(k) if what != 'start' else ''} sums to {sums[k]!r}, not 1")

    def _start(self, stmt, sn):
        S = len(sn)
        if stmt is None:
            return np.full(S, 1.0 / S), self.last_line
        kw, line, rest, toks = stmt
        words = [(t, line) for t in rest.split()] + list(toks)
        if not words:
            raise ValueError(f"line {line}: `{kw}:` needs a value")
        if kw == "start":
            if len(words) == 1 and words[0][0] == "uniform":
                return np.full(S, 1.0 / S), line
            one_state = len(words) == 1 and (S > 1 or words[0][0] in sn)
            if not one_state:
                if len(words) != S:
                    raise ValueError(f"line {words[-1][1]}: `start:` needs {S} probabilities, `uniform` or one state; found {len(words)} values")
                return np.array([self._prob(t, ln) for t, ln in words]), words[-1][1]
        chosen = np.zeros(S, dtype=bool)
        for t, ln in words:
            k = self._index(t, sn, "state", ln)
            if isinstance(k, slice):
                raise ValueError(f"line {ln}: `*` is not a start state")
            chosen[k] = True
        if kw == "start exclude":
            chosen = ~chosen
        if not chosen.any():
            raise ValueError(f"line {line}: `{kw}:` leaves no start state")
        return chosen / chosen.sum(), line

    def _values(self, vals, count, line, prob):
        if len(vals) != count:
            raise ValueError(f"line {vals[-1][1] if vals else line}: expected {count} values, found {len(vals)}")
        conv = self._prob if prob else self._number
        return np.array([conv(t, ln) for t, ln in vals])

    def _entry_T(self, idx, vals, line, T, D, t_line, sn, an):
        A, S = D.shape
        a = self._index(idx[0], an, "action", line)
        end = vals[-1][1] if vals else line
        if len(idx) == 1:
            word = vals[0][0] if len(vals) == 1 else None
            if word == "uniform":
                m = np.full((S, S), 1.0 / S)
            elif word == "identity":
                m = np.eye(S)
            else:
                m = self._values(vals, S * S, line, True).reshape(S, S)
            T[a], D[a], t_line[a] = m, False, end
        elif len(idx) == 2:
            s = self._index(idx[1], sn, "state", line)
            word = vals[0][0] if len(vals) == 1 else None
            if word == "reset":
                T[a, s], D[a, s], t_line[a, s] = 0.0, True, end
                return
            row = np.full(S, 1.0 / S) if word == "uniform" else self._values(vals, S, line, True)
            T[a, s], D[a, s], t_line[a, s] = row, False, end
        elif len(idx) == 3:
            s, s2 = self._index(idx[1], sn, "state", line), self._index(idx[2], sn, "state", line)
            p = self._values(vals, 1, line, True)[0]
            was = np.array(D[a, s], copy=True)
            if was.any():                                         # an overridden reset pair starts from an empty row
                T[a, s] = np.where(was[..., None], 0.0, T[a, s])
            T[a, s, s2], D[a, s], t_line[a, s] = p, False, end
        else:
            raise ValueError(f"line {line}: `T:` takes 1 to 3 indices")

    def _entry_O(self, idx, vals, line, O, o_line, sn, an, zn):
        A, S, Z = O.shape
        a = self._index(idx[0], an, "action", line)
        end = vals[-1][1] if vals else line
        if len(idx) == 1:
            word = vals[0][0] if len(vals) == 1 else None
            O[a] = np.full((S, Z), 1.0 / Z) if word == "uniform" else self._values(vals, S * Z, line, True).reshape(S, Z)
            o_line[a] = end
        elif len(idx) == 2:
            s2 = self._index(idx[1], sn, "state", line)
            word = vals[0][0] if len(vals) == 1 else None
            O[a, s2] = np.full(Z, 1.0 / Z) if word == "uniform" else self._values(vals, Z, line, True)
            o_line[a, s2] = end
        elif len(idx) == 3:
            s2, z = self._index(idx[1], sn, "state", line), self._index(idx[2], zn, "observation", line)
            O[a, s2, z] = self._values(vals, 1, line, True)[0]
            o_line[a, s2] = end
        else:
            raise ValueError(f"line {line}: `O:` takes 1 to 3 indices")

    def _entry_R(self, idx, vals, line, R, sn, an, zn):
        A, S, _, Z = R.shape
        if len(idx) < 2 or len(idx) > 4:
            raise ValueError(f"line {line}: `R:` takes 2 to 4 indices")
        a, s = self._index(idx[0], an, "action", line), self._index(idx[1], sn, "state", line)
        if len(idx) == 2:
            R[a, s] = self._values(vals, S * Z, line, False).reshape(S, Z)
        elif len(idx) == 3:
            R[a, s, self._index(idx[2], sn, "state", line)] = self._values(vals, Z, line, False)
        else:
            R[a, s, self._index(idx[2], sn, "state", line), self._index(idx[3], zn, "observation", line)] = self._values(vals, 1, line, False)[0]


def load_pomdp(path_or_text) -> PomdpModel:
    """A `.pomdp` file (a path) or its text (anything with a newline or a colon that is not an existing file) -> PomdpModel."""
    text = str(path_or_text)
    if "\n" not in text and (os.path.exists(text) or text.endswith(".pomdp")):
        with open(text) as f:
            text = f.read()
    return _Parser(text).parse()
