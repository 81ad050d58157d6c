"""Voice prefix cache: the slow-stack KV of a reference voice's system message, kept on the device
and copied into a request's slot instead of being prefilled again (server flag --voice-cache-mb).

Every voice-cloning request starts its prompt with the same system message (instruction text,
reference transcripts, reference codes: fishmi.prompt.base_conversation).  The cache holds, per
distinct message, the (C+1, P) token block and the id of a device snapshot of the KV rows [0, P)
those tokens produce (DualARModel.save_prefix); a later request whose prompt starts with the same
block loads the rows into its slot (load_prefix) and prefills only the rest at pos0 = P.

Entries are addressed by content: the key is a digest of the token block, and a hit is confirmed by
comparing the tokens themselves.  Nothing is invalidated by reference_id: an edited or deleted
reference encodes to other codes, hence to another key, and the stale entry ages out (least
recently used first) once max_bytes is reached.  One instance per model, used from the worker
thread that owns the model.
"""
from __future__ import annotations

import collections
import hashlib
import logging
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import native

log = logging.getLogger("fishmi.prefix_cache")


@dataclass(eq=False)
class PrefixEntry:
    tokens: np.ndarray  # (C+1, P) int32: the block whose KV the snapshot holds
    pid: int            # the model's prefix id
    nbytes: int         # device bytes of the snapshot

    @property
    def P(self) -> int:
        return self.tokens.shape[1]


def _key(tokens: np.ndarray) -> bytes:
    h = hashlib.blake2b(digest_size=16)
    h.update(repr(tokens.shape).encode())
    h.update(tokens.tobytes())
    return h.digest()


class PrefixCache:
    def __init__(self, model, max_bytes: int, min_positions: int = 32):
        self.m = model
        self.max_bytes = int(max_bytes)
        self.min_positions = int(min_positions)
        self.entries: "collections.OrderedDict[bytes, PrefixEntry]" = collections.OrderedDict()  # LRU first
        self.stats = {"hits": 0, "misses": 0, "inserts": 0, "evictions": 0, "failures": 0, "bytes": 0}

    @staticmethod
    def _block(tokens) -> np.ndarray:
        return np.ascontiguousarray(tokens, dtype=np.int32)

    def _find(self, block: np.ndarray) -> Optional[PrefixEntry]:
        e = self.entries.get(_key(block))
        if e is not None and e.tokens.shape == block.shape and np.array_equal(e.tokens, block):
            return e
        return None

    def holds(self, entry: PrefixEntry) -> bool:
        """Whether `entry` (from an earlier lookup) is still stored."""
        return self.entries.get(_key(entry.tokens)) is entry

    def lookup(self, enc) -> Optional[PrefixEntry]:
        """The longest entry that is a column prefix of the prompt `enc` (C+1, T) and leaves at least
        one position to prefill (P <= T - 1); None on a miss."""
        enc = np.asarray(enc)
        T = enc.shape[1]
        for P in sorted({e.P for e in self.entries.values()}, reverse=True):
            if P > T - 1:
                continue
            e = self._find(self._block(enc[:, :P]))
            if e is not None:
                self.entries.move_to_end(_key(e.tokens))
                self.stats["hits"] += 1
                return e
        self.stats["misses"] += 1
        return None

    def insert(self, slot: int, tokens) -> Optional[PrefixEntry]:
        """Store the block `tokens` (C+1, P) whose KV `slot` holds at positions [0, P).  Returns the
        entry (the existing one when the block is already present), or None when it is not stored:
        shorter than min_positions, larger than max_bytes, or the device could not allocate it."""
        block = self._block(tokens)
        P = block.shape[1]
        e = self._find(block)
        if e is not None:
            return e
        if P < max(1, self.min_positions):
            return None
        need = int(self.m.prefix_bytes(P))
        if need > self.max_bytes:
            return None
        while self.entries and self.stats["bytes"] + need > self.max_bytes:
            self._evict()
        try:
            pid = self.m.save_prefix(slot, P)
        except native.FishMIError as err:
            if err.code != native.FM_ERR_OOM:
                raise
            self.stats["failures"] += 1
            log.warning("voice prefix of %d positions not cached: %s", P, err)
            return None
        e = PrefixEntry(block.copy(), pid, int(self.m.prefix_info(pid)[1]))
        self.entries[_key(block)] = e
        self.stats["inserts"] += 1
        self.stats["bytes"] += e.nbytes
        return e

    def _evict(self):
        _, e = self.entries.popitem(last=False)
        self.m.drop_prefix(e.pid)
        self.stats["evictions"] += 1
        self.stats["bytes"] -= e.nbytes

    def close(self):
        while self.entries:
            _, e = self.entries.popitem(last=False)
            self.m.drop_prefix(e.pid)
            self.stats["bytes"] -= e.nbytes
