"""Host-side mirror of ``pyopal.lib`` for the MI355X search path.

Same names, argument meaning and error behaviour as the reference's Cython
module (``src/pyopal/lib.pyx``); the computation behind `Aligner.align` is the
HIP path reached through the C ABI (``pyopal_amd._capi``), never a CPU
fallback. Per-residue loops of the reference (encoding, result fill) are
numpy table look-ups / bulk array reads here.
"""

from __future__ import annotations

import array
import threading
import typing
import weakref

import numpy as np

from . import _capi
from .matrices import ScoringMatrix

__version__ = "0.1.0"

MAX_ALPHABET_SIZE = 32  # src/pyopal/lib.pxd:28-32
UINT32_MAX = 0xFFFFFFFF

_OPAL_SEARCH_MODES = dict(_capi.SEARCH)        # src/pyopal/lib.pyx:73-77
_OPAL_OVERFLOW_MODES = dict(_capi.OVERFLOW)    # src/pyopal/lib.pyx:85-88
_OPAL_ALGORITHMS = dict(_capi.MODE)            # src/pyopal/lib.pyx:90-95
_OPAL_ALIGNMENT_OPERATION = {"M": 0, "D": 1, "I": 2, "X": 3}  # src/pyopal/lib.pyx:97-102


# --- Read/write lock ------------------------------------------------------------

class SharedMutex:
    """Readers-writer lock with the surface of ``src/pyopal/lib.pyx:153-181``
    (``lock.read`` / ``lock.write`` context managers). Searches hold the read
    side while the C call runs without the GIL; mutators hold the write side."""

    def __init__(self):
        self._cond = threading.Condition(threading.Lock())
        self._readers = 0
        self._writer = False
        self.read = ReadLock(self)
        self.write = WriteLock(self)


class ReadLock:
    def __init__(self, owner: SharedMutex):
        self.owner = owner

    def __enter__(self):
        o = self.owner
        with o._cond:
            while o._writer:
                o._cond.wait()
            o._readers += 1

    def __exit__(self, exc_type, exc_value, traceback):
        o = self.owner
        with o._cond:
            o._readers -= 1
            if o._readers == 0:
                o._cond.notify_all()


class WriteLock:
    def __init__(self, owner: SharedMutex):
        self.owner = owner

    def __enter__(self):
        o = self.owner
        with o._cond:
            while o._writer or o._readers:
                o._cond.wait()
            o._writer = True

    def __exit__(self, exc_type, exc_value, traceback):
        o = self.owner
        with o._cond:
            o._writer = False
            o._cond.notify_all()


# --- Alphabet -------------------------------------------------------------------

class Alphabet:
    """Ordinal encoding of sequences (``src/pyopal/lib.pyx:186-332``).

    Letters outside the alphabet (lower case included: there is no case
    folding) map to the index of ``*``; non-letters are rejected.
    """

    _DEFAULT_LETTERS = "ARNDCQEGHILKMFPSTWYVBZX*"
    __slots__ = ("letters", "length", "_unknown", "_table", "_trans", "_letters")

    def __init__(self, letters: str = _DEFAULT_LETTERS):
        if not isinstance(letters, str):
            raise TypeError(f"expected str, found {type(letters).__name__}")
        if len(letters) != len(set(letters)):
            raise ValueError("duplicate symbols in alphabet letters")
        if any(x != "*" and not x.isupper() for x in letters):
            raise ValueError("alphabet must only contain uppercase characters or wildcard")
        if len(letters) > MAX_ALPHABET_SIZE:
            raise ValueError("Cannot use alphabet of more than 32 symbols")
        self.letters = letters
        self.length = len(letters)
        self._unknown = letters.find("*")
        self._letters = np.frombuffer(letters.encode("ascii"), dtype=np.uint8).copy()
        # 255: not a letter; 254: letter without a code (alphabet has no wildcard)
        table = np.full(256, 255, dtype=np.uint8)
        for c in range(256):
            if (65 <= c <= 90) or (97 <= c <= 122):
                table[c] = self._unknown if self._unknown >= 0 else 254
        for i, x in enumerate(self._letters):
            if (65 <= x <= 90) or (97 <= x <= 122):
                table[x] = i
        self._table = table
        self._trans = table.tobytes()  # 256-entry table for bytes.translate

    def __len__(self):
        return self.length

    def __contains__(self, item):
        return item in self.letters

    def __getitem__(self, index: int):
        index_ = index
        if index_ < 0:
            index_ += self.length
        if index_ < 0 or index_ >= self.length:
            raise IndexError(index)
        return self.letters[index_]

    def __reduce__(self):
        return type(self), (self.letters,)

    def __repr__(self):
        if self.letters == self._DEFAULT_LETTERS:
            return f"{type(self).__name__}()"
        return f"{type(self).__name__}({self.letters!r})"

    def __str__(self):
        return self.letters

    def __eq__(self, item):
        if isinstance(item, str):
            return self.letters == item
        if isinstance(item, Alphabet):
            return self.letters == item.letters
        return False

    def __hash__(self):
        return hash(self.letters)

    # -- bulk forms used by Database --------------------------------------------
    def _encode_bytes(self, sequence) -> bytes:
        """Ordinal encoding of a str / bytes-like sequence in one C-level pass."""
        if isinstance(sequence, str):
            sequence = sequence.encode("ascii", "replace")
        elif not isinstance(sequence, (bytes, bytearray)):
            sequence = memoryview(sequence).cast("B").tobytes()
        codes = sequence.translate(self._trans)
        if b"\xff" in codes or b"\xfe" in codes:
            bad = [p for p in (codes.find(b"\xff"), codes.find(b"\xfe")) if p >= 0]
            pos = min(bad)
            letter = sequence[pos]
            if codes[pos] == 255:
                raise ValueError(f"character outside ASCII range: {letter!r}")
            raise ValueError(f"non-alphabet character in sequence: {chr(letter)!r}")
        return bytes(codes)

    def _encode_array(self, sequence) -> np.ndarray:
        return np.frombuffer(self._encode_bytes(sequence), dtype=np.uint8)

    def encode_into(self, sequence, encoded) -> None:
        src = memoryview(sequence).cast("B")
        dst = memoryview(encoded).cast("B")
        if len(src) != len(dst):
            raise ValueError("Buffers do not have the same dimensions")
        dst[:] = self._encode_bytes(src)

    def decode_into(self, encoded, sequence) -> None:
        src = np.frombuffer(memoryview(encoded).cast("B"), dtype=np.uint8)
        dst = memoryview(sequence).cast("B")
        if len(src) != len(dst):
            raise ValueError("Buffers do not have the same dimensions")
        if src.size and src.max() >= self.length:
            code = int(src[np.argmax(src >= self.length)])
            raise ValueError(f"invalid index in encoded sequence: {code!r}")
        dst[:] = self._letters[src].tobytes()

    def encode(self, sequence) -> bytes:
        return self._encode_bytes(sequence)

    def decode(self, encoded) -> str:
        decoded = bytearray(len(encoded))
        self.decode_into(encoded, decoded)
        return decoded.decode("ascii")


# --- Sequence storage -------------------------------------------------------------

class BaseDatabase:
    """Base class of sequence databases (``src/pyopal/lib.pyx:337-466``).

    The reference's three C-level accessors (``get_sequences``/``get_lengths``/
    ``get_size``, ``src/pyopal/lib.pxd:90-92``) become `_get_size`,
    `_get_lengths` and `_get_encoded`; a subclass that implements them can be
    searched by `Aligner.align`.
    """

    _DEFAULT_ALPHABET = Alphabet()

    def __init__(self, sequences=(), alphabet=None):
        self.lock = SharedMutex()
        self._mirrors: typing.Dict[int, typing.Tuple[int, _capi.DeviceDatabase]] = {}
        self._mirror_guard = threading.Lock()
        self._version = 0
        if alphabet is None:
            self.alphabet = self._DEFAULT_ALPHABET
        elif isinstance(alphabet, Alphabet):
            self.alphabet = alphabet
        else:
            self.alphabet = Alphabet(alphabet)
        if sequences:
            raise TypeError("cannot create a `BaseDatabase` with sequences")

    # -- interface to implement ---------------------------------------------------
    def _get_size(self) -> int:
        return 0

    def _get_lengths(self) -> typing.Sequence[int]:
        raise NotImplementedError("BaseDatabase.get_lengths")

    def _get_encoded(self) -> typing.Sequence[bytes]:
        raise NotImplementedError("BaseDatabase.get_sequences")

    # -- device mirror -----------------------------------
    def _device_mirror(self, device: int = 0,
                       shard: typing.Optional[typing.Tuple[int, int]] = None) -> _capi.DeviceDatabase:
        """Packed copy of the database - or of its targets ``[lo, hi)`` only, when ``shard`` is
        given (`pyopal_amd.align` on several GPUs: every GPU holds 1/N of the residues) - in the
        HBM of ``device``, rebuilt only after a mutation. Called with the read lock held."""
        key = (device, shard)
        with self._mirror_guard:
            # mirrors of an older state of the database are dropped whichever is asked for
            for old in [k for k, (version, _) in self._mirrors.items() if version != self._version]:
                self._mirrors.pop(old)[1].close()
            entry = self._mirrors.get(key)
            if entry is not None:
                return entry[1]
            derived = self._mirror_from_parent(device) if shard is None else None
            if derived is not None:
                self._mirrors[key] = (self._version, derived)
                return derived
            seqs = self._get_encoded()
            lo, hi = (0, len(seqs)) if shard is None else shard
            if not 0 <= lo <= hi <= len(seqs):
                raise IndexError(f"shard [{lo}, {hi}) outside the database")
            if shard is not None:
                seqs = seqs[lo:hi]
            lengths = np.fromiter(self._get_lengths(), dtype=np.int64)[lo:hi]
            offsets = np.zeros(len(seqs) + 1, dtype=np.int64)
            np.cumsum(lengths, out=offsets[1:])
            residues = np.frombuffer(b"".join(seqs), dtype=np.uint8)
            mirror = _capi.DeviceDatabase(residues, offsets, self.alphabet.length, device)
            self._mirrors[key] = (self._version, mirror)
            return mirror

    def _mirror_from_parent(self, device: int):
        """A subset made by `Database.mask` / `Database.extract` whose parent is still resident on
        ``device`` and unchanged gathers its residues there from the parent's mirror instead of
        uploading them again (the reference's subsets share the parent's
        sequence buffers, ``src/pyopal/lib.pyx:694-778``). None: build the mirror the ordinary way."""
        link = getattr(self, "_parent_link", None)
        if link is None:
            return None
        parent_ref, parent_version, my_version, indices = link
        parent = parent_ref()
        if parent is None or my_version != self._version:
            self._parent_link = None     # the parent is gone, or this subset was edited: nothing to share
            return None
        with parent._mirror_guard:
            entry = parent._mirrors.get((device, None))
            if entry is None or entry[0] != parent_version or parent._version != parent_version:
                return None
            return entry[1].subset(indices)

    def _invalidate(self) -> None:
        """Called with the write lock held by every mutator."""
        self._version += 1

    # -- properties -----------------------------------------------------------------
    @property
    def lengths(self) -> typing.List[int]:
        with self.lock.read:
            return [int(x) for x in self._get_lengths()][: self._get_size()]

    @property
    def total_length(self) -> int:
        with self.lock.read:
            if self._get_size() == 0:
                return 0
            return int(sum(self._get_lengths()))

    # -- sequence interface ---------------------------------------------------------
    def __contains__(self, query):
        encoded = self.alphabet.encode(query)
        with self.lock.read:
            if self._get_size() == 0:
                return False
            return any(s == encoded for s in self._get_encoded())

    def __len__(self):
        with self.lock.read:
            return self._get_size()

    def __getitem__(self, index: int):
        with self.lock.read:
            size = self._get_size()
            index_ = index
            if index_ < 0:
                index_ += size
            if index_ < 0 or index_ >= size:
                raise IndexError(index)
            return self.alphabet.decode(self._get_encoded()[index_])


class Database(BaseDatabase):
    """A database of target sequences, stored encoded
    (``src/pyopal/lib.pyx:469-778``)."""

    def __init__(self, sequences=(), alphabet=None):
        super().__init__(alphabet=alphabet)
        self._sequences: typing.List[bytes] = []
        self._lengths: typing.List[int] = []
        self.clear()
        self.extend(sequences)

    def __reduce__(self):
        return (type(self), ((), self.alphabet), None, iter(self))

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    # -- database interface -----------------------------------------------------------
    def _get_size(self) -> int:
        return len(self._sequences)

    def _get_lengths(self):
        return self._lengths

    def _get_encoded(self):
        return self._sequences

    def _encode(self, sequence) -> bytes:
        return self.alphabet.encode(sequence)

    # -- sequence interface -----------------------------------------------------------
    def __getitem__(self, index):
        if isinstance(index, slice):
            return self.extract(range(*index.indices(len(self))))
        return super().__getitem__(index)

    def __setitem__(self, index: int, sequence):
        encoded = self._encode(sequence)
        with self.lock.write:
            size = len(self._sequences)
            index_ = index
            if index_ < 0:
                index_ += size
            if index_ < 0 or index_ >= size:
                raise IndexError(index)
            self._sequences[index_] = encoded
            self._lengths[index_] = len(encoded)
            self._invalidate()

    def __delitem__(self, index: int):
        with self.lock.write:
            size = len(self._sequences)
            index_ = index
            if index_ < 0:
                index_ += size
            if index_ < 0 or index_ >= size:
                raise IndexError(index)
            del self._sequences[index_]
            del self._lengths[index_]
            self._invalidate()

    def clear(self) -> None:
        with self.lock.write:
            self._sequences.clear()
            self._lengths.clear()
            self._invalidate()

    def extend(self, sequences) -> None:
        # Bulk path (the reference encodes sequence by sequence, lib.pyx:586-636; here one
        # table look-up over the concatenation replaces a Python-level loop per residue):
        # lists of str / bytes are joined, encoded once and cut back at their lengths.
        if isinstance(sequences, (list, tuple)) and len(sequences) > 8:
            if all(type(x) is str for x in sequences):
                joined = "".join(sequences).encode("ascii", "replace")
            elif all(type(x) is bytes for x in sequences):
                joined = b"".join(sequences)
            else:
                joined = None
            if joined is not None:
                lengths = [len(x) for x in sequences]
                try:
                    encoded = self.alphabet.encode(joined)
                except ValueError:
                    encoded = None  # let the per-sequence path raise for the offending one
                if encoded is not None and len(encoded) == sum(lengths):
                    pieces = []
                    offset = 0
                    for n in lengths:
                        pieces.append(encoded[offset:offset + n])
                        offset += n
                    with self.lock.write:
                        self._sequences.extend(pieces)
                        self._lengths.extend(lengths)
                        self._invalidate()
                    return
        for sequence in sequences:
            self.append(sequence)

    def append(self, sequence) -> None:
        encoded = self._encode(sequence)
        with self.lock.write:
            self._sequences.append(encoded)
            self._lengths.append(len(encoded))
            self._invalidate()

    def reverse(self) -> None:
        with self.lock.write:
            self._sequences.reverse()
            self._lengths.reverse()
            self._invalidate()

    def insert(self, index: int, sequence) -> None:
        encoded = self._encode(sequence)
        with self.lock.write:
            size = len(self._sequences)
            index_ = index
            if index_ < 0:
                index_ += size
            if index_ < 0:
                index_ = 0
            elif index_ >= size:
                index_ = size
            self._sequences.insert(index_, encoded)
            self._lengths.insert(index_, len(encoded))
            self._invalidate()

    # -- subsets (share the encoded buffers, like the reference's shared_ptr) ------------
    def _subset(self) -> "Database":
        subdb = Database.__new__(Database)
        BaseDatabase.__init__(subdb, alphabet=self.alphabet)
        subdb._sequences = []
        subdb._lengths = []
        return subdb

    def _link_subset(self, subdb: "Database", picked: typing.List[int]) -> None:
        """(read lock held) Remember where the subset came from: while this database and the subset
        stay as they are, the subset's device mirror is gathered from this one's on the device."""
        picked = np.asarray(picked, dtype=np.int64)
        link = getattr(self, "_parent_link", None)
        if link is not None and link[2] == self._version and link[0]() is not None:
            # a subset of an (unedited) subset: linked to the database at the root, which is the one
            # likely to be resident
            subdb._parent_link = (link[0], link[1], subdb._version, link[3][picked])
        else:
            subdb._parent_link = (weakref.ref(self), self._version, subdb._version, picked)

    def mask(self, bitmask) -> "Database":
        subdb = self._subset()
        picked = []
        with self.lock.read:
            size = self._get_size()
            i = 0
            for b in bitmask:
                if i >= size:
                    raise IndexError(bitmask)
                if b:
                    subdb._sequences.append(self._sequences[i])
                    subdb._lengths.append(self._lengths[i])
                    picked.append(i)
                i += 1
            if i < size:
                raise IndexError(bitmask)
            self._link_subset(subdb, picked)
        return subdb

    def extract(self, indices) -> "Database":
        subdb = self._subset()
        picked = []
        with self.lock.read:
            size = self._get_size()
            for index in indices:
                if index < 0 or index >= size:
                    raise IndexError(index)
                subdb._sequences.append(self._sequences[index])
                subdb._lengths.append(self._lengths[index])
                picked.append(index)
            self._link_subset(subdb, picked)
        return subdb


# --- Results ----------------------------------------------------------------------

# Cython, like the reference's (src/pyopal/lib.pyx:783-1119): see _results.pyx
try:
    from ._results import EndResult, FullResult, ScoreResult  # noqa: E402
except ImportError as err:  # pragma: no cover
    raise ImportError(
        "pyopal_amd._results is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
        "(or `make -C pyopal_amd/csrc`)") from err

_RESULT_TYPES = {"score": ScoreResult, "end": EndResult, "full": FullResult}


def _empty_arrays(mode: str, shape=(0,), fill: int = 0) -> typing.Dict[str, np.ndarray]:
    """The arrays of a search that had nothing to do, with the keys and dtypes the device calls give them: "score",
    for "end" and "full" also "end_q" / "end_t", for "full" (no entries then) also "start_q" / "start_t" and no
    operations behind one offset."""
    out = {"score": np.full(shape, fill, dtype=np.int32)}
    if mode != "score":
        out.update(end_q=np.full(shape, fill, dtype=np.int32), end_t=np.full(shape, fill, dtype=np.int32))
    if mode == "full":
        out.update(start_q=np.zeros(0, dtype=np.int32), start_t=np.zeros(0, dtype=np.int32),
                   aln_flat=np.zeros(0, dtype=np.uint8), aln_off=np.zeros(1, dtype=np.int64))
    return out


def _result_objects(mode: str, target, query, query_lengths, target_lengths, out) -> typing.List[ScoreResult]:
    """Arrays as result objects, one per entry: ``target`` the target index of every entry, ``query`` the index of its
    query in ``query_lengths``, ``target_lengths`` one per target of the database (``query`` and the lengths are only
    read for "full"), ``out`` the arrays of a device call with one entry each."""
    score = out["score"].tolist()
    target = np.asarray(target).tolist()
    if mode == "score":
        return [ScoreResult(t, s) for t, s in zip(target, score)]
    end_q, end_t = out["end_q"].tolist(), out["end_t"].tolist()
    if mode == "end":
        return [EndResult(t, s, qe, te) for t, s, qe, te in zip(target, score, end_q, end_t)]
    start_q, start_t = out["start_q"].tolist(), out["start_t"].tolist()
    off = out["aln_off"].tolist()
    text = out["aln_flat"].tobytes().translate(_OPS_TO_TEXT).decode("ascii")
    return [FullResult(t, score[p], end_q[p], end_t[p], start_q[p], start_t[p], query_lengths[q], int(target_lengths[t]),
                       text[off[p]:off[p + 1]])
            for p, (q, t) in enumerate(zip(np.asarray(query).tolist(), target))]


def _target_lengths(mirror, mode: str):
    """what `_result_objects` reads of the targets: for "full" their lengths, otherwise nothing"""
    return np.diff(mirror.offsets) if mode == "full" and mirror is not None else None


def _cut(flat: list, counts: typing.List[int]) -> typing.List[list]:
    """``flat`` cut into one list per entry of ``counts``"""
    out, lo = [], 0
    for c in counts:
        out.append(flat[lo:lo + c])
        lo += c
    return out


def _count_argument(name: str, value, low: int, high: int, limit: str) -> int:
    """``k`` of the top hits, ``m`` of the best queries"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{name} must be an integer, not {type(value).__name__}")
    if value < low or value > high:
        raise ValueError(f"{name} must be between {low} and {high} ({limit}), got {int(value)}")
    return int(value)


def _max_hits_argument(max_hits) -> typing.Optional[int]:
    if max_hits is None:
        return None
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)):
        raise TypeError(f"max_hits must be an integer or None, not {type(max_hits).__name__}")
    if max_hits < 0:
        raise ValueError("max_hits must not be negative")
    return int(max_hits)


# --- The query side and the preamble of Aligner's extension entry points ----------------

class _QuerySide:
    """What an extension entry point of `Aligner` searches with: one sequence or a list of them with the aligner's
    matrix (`_Sequences`), one `Pssm` or a list of them (`_Profiles`). It makes the checks that depend on which it is,
    and the device calls: ``on(mirror)`` is its counterpart in `_capi`, which the selections take; their answers
    come back in one shape, a row or a CSR segment per query, whether the queries are one or many."""

    __slots__ = ("aligner", "given", "many", "lengths")

    def __init__(self, aligner: "Aligner", given, many: bool):
        self.aligner, self.given, self.many = aligner, given, many
        self.lengths = None     # one per query, once `check` has run

    def per_query(self, values: np.ndarray):
        """one value per query (thresholds, E-value cuts) as the device call takes it: the array, or the one number"""
        return values if self.many else values[0].item()

    def top(self, mirror, mode, algorithm, start, end, k, min_score):
        """(the count of every query, {"target", "score", "end_t" / "end_q": tables of shape (queries, k)})"""
        out = mirror._search_top(self.on(mirror), mode, algorithm, start, end, k, min_score)
        counts = out.pop("count")
        if self.many:
            return counts.tolist(), out
        return [counts], {key: table[None, :] for key, table in out.items()}

    def hits(self, mirror, mode, algorithm, start, end, thresholds, max_hits) -> typing.Dict[str, typing.Any]:
        """the CSR of `DeviceDatabase.search_batch_hits`"""
        return self._csr(mirror._search_hits(self.on(mirror), mode, algorithm, start, end, self.per_query(thresholds),
                                             max_hits))

    def significant(self, mirror, mode, algorithm, start, end, cuts, exclude_z, max_hits) -> typing.Dict[str, typing.Any]:
        """the CSR of `DeviceDatabase.search_batch_significant`, "fits" a list of `ScoreFit`"""
        out = self._csr(mirror._search_significant(self.on(mirror), mode, algorithm, start, end, self.per_query(cuts),
                                                   exclude_z, max_hits))
        out.pop("_fits_owner", None)
        out["fits"] = [ScoreFit(f) for f in out["fits"]]
        return out

    def _csr(self, out):
        if not self.many:
            out["offsets"] = np.array([0, out.pop("count")], dtype=np.int64)
            if "fit" in out:
                out["fits"] = [out.pop("fit")]
        return out


class _Sequences(_QuerySide):
    __slots__ = ("arrays",)
    pair_index, pair_outside = "query_index", "query index of a pair outside the queries"

    def check_type(self) -> None:
        pass

    def check(self, database: "BaseDatabase") -> None:
        if database.alphabet != self.aligner.alphabet:
            raise ValueError("database and score matrix have different alphabets")
        queries = list(self.given) if self.many else [self.given]
        for q in queries:
            if q is None:
                raise TypeError("Argument 'query' must not be None")
        self.arrays = [np.frombuffer(database.alphabet.encode(q), dtype=np.uint8) for q in queries]
        self.lengths = [len(a) for a in self.arrays]

    @property
    def codes(self) -> np.ndarray:
        return self.arrays[0]

    def on(self, mirror):
        a = self.aligner
        if self.many:
            return mirror._batch_side(self.arrays, a._matrix, a.gap_open, a.gap_extend)
        return mirror._query_side(self.arrays[0], a._matrix, a.gap_open, a.gap_extend)

    def search(self, mirror, mode, algorithm, start, end):
        a = self.aligner
        if self.many:
            return mirror.search_batch(self.arrays, a._matrix, a.gap_open, a.gap_extend, mode, algorithm, start, end)
        return mirror.search(self.arrays[0], a._matrix, a.gap_open, a.gap_extend, mode, algorithm, start, end)

    def align_pairs(self, mirror, pair_query, pair_target, mode, algorithm):
        a = self.aligner
        return mirror.align_pairs(self.arrays, pair_query, pair_target, a._matrix, a.gap_open, a.gap_extend, mode, algorithm)

    def profile_columns(self, mirror, targets, algorithm, return_msa):
        a = self.aligner
        return mirror.profile_columns(self.arrays[0], a._matrix, targets, a.gap_open, a.gap_extend, algorithm, return_msa)


class _Profiles(_QuerySide):
    __slots__ = ("pssms",)
    pair_index, pair_outside = "pssm_index", "PSSM index of a pair outside the PSSMs"

    def check_type(self) -> None:
        if self.many:
            self.pssms = list(self.given)
            for pssm in self.pssms:
                if not isinstance(pssm, Pssm):
                    raise TypeError("Argument 'pssms' has an item of incorrect type (expected Pssm, got "
                                    f"{type(pssm).__name__})")
        else:
            if not isinstance(self.given, Pssm):
                raise TypeError(f"Argument 'pssm' has incorrect type (expected Pssm, got {type(self.given).__name__})")
            self.pssms = [self.given]

    def check(self, database: "BaseDatabase") -> None:
        for pssm in self.pssms:
            if pssm.alphabet != database.alphabet:
                raise ValueError("database and PSSM have different alphabets")
        self.lengths = [len(pssm) for pssm in self.pssms]

    @property
    def codes(self) -> np.ndarray:
        return self.pssms[0].consensus

    def on(self, mirror):
        return mirror._pssm_side(self.pssms[0].scores, None, self.aligner.gap_open, self.aligner.gap_extend)

    @property
    def arrays(self) -> typing.List[np.ndarray]:
        return [p.scores for p in self.pssms]

    def search(self, mirror, mode, algorithm, start, end):
        pssm = self.pssms[0]
        return mirror.search_pssm(pssm.scores, pssm.consensus, self.aligner.gap_open, self.aligner.gap_extend, mode,
                                  algorithm, start, end)

    def align_pairs(self, mirror, pair_pssm, pair_target, mode, algorithm):
        return mirror.align_pairs_pssm([p.scores for p in self.pssms], [p.consensus for p in self.pssms], pair_pssm,
                                       pair_target, self.aligner.gap_open, self.aligner.gap_extend, mode, algorithm)

    def profile_columns(self, mirror, targets, algorithm, return_msa):
        pssm = self.pssms[0]
        return mirror.profile_columns_pssm(pssm.scores, pssm.consensus, targets, self.aligner.gap_open,
                                           self.aligner.gap_extend, algorithm, return_msa)


class _Request:
    """The preamble of every extension entry point of `Aligner` (`align` keeps the reference's own, check for check).
    Its checks, in this order:

    1. the type of a `Pssm` argument;
    2. ``mode`` (None: the method has none), then ``algorithm``;
    3. the method's own count argument (``k``, ``m``, ``max_hits``): ``check()``, whose answer is kept as ``checked``;
    4. a negative ``start`` or ``end``;
    5. the type of the database;
    6. its alphabet against the matrix's or the PSSM's;
    7. no query is None; the queries are encoded;
    8. what the method has per query or per entry (thresholds, E-value cuts, pairs, targets): by the method, before
       it enters the request;
    9. entering the request takes the database's read lock and checks the slice: an end below the start, the clamp
       to the size, a start past the end.

    Inside the ``with`` block ``start`` and ``end`` are the clamped slice, ``size`` the database's, and ``mirror()`` the
    device mirror - asked for only when there is something to compute, so that an empty request needs no device."""

    __slots__ = ("database", "start", "end", "size", "device", "checked", "_mirror")

    def __init__(self, side: _QuerySide, database: "BaseDatabase", mode: typing.Optional[str], algorithm: str,
                 start: int = 0, end: int = UINT32_MAX, device: int = 0, check: typing.Optional[typing.Callable] = None):
        side.check_type()
        if mode is not None and mode not in _OPAL_SEARCH_MODES:
            raise ValueError(f"invalid search mode: {mode!r}")
        if algorithm not in _OPAL_ALGORITHMS:
            raise ValueError(f"invalid algorithm: {algorithm!r}")
        self.checked = None if check is None else check()
        if start < 0 or end < 0:
            raise OverflowError("can't convert negative value to uint32_t")
        if not isinstance(database, BaseDatabase):
            raise TypeError(f"Argument 'database' has incorrect type (expected BaseDatabase, "
                            f"got {type(database).__name__})")
        side.check(database)
        self.database, self.start, self.end, self.device = database, start, end, device
        self._mirror = None

    def __enter__(self) -> "_Request":
        self.database.lock.read.__enter__()
        try:
            self.size = self.database._get_size()
            if self.end < self.start:
                raise IndexError("database slice end is lower than start")
            self.end = min(self.end, self.size)
            if self.start > self.size:
                raise IndexError("database slice start is past the end of the database")
        except BaseException:
            self.database.lock.read.__exit__(None, None, None)
            raise
        return self

    def __exit__(self, exc_type, exc_value, traceback):
        self.database.lock.read.__exit__(exc_type, exc_value, traceback)

    def mirror(self) -> _capi.DeviceDatabase:
        if self._mirror is None:
            if _capi.lib().miopalDeviceCount() < 1:
                raise RuntimeError("no supported SIMD backend available")
            self._mirror = self.database._device_mirror(self.device)
        return self._mirror


# --- Aligner ------------------------------------------------------------------------

def resolve_scoring_matrix(spec, verb: str = "found") -> ScoringMatrix:
    """``None`` (BLOSUM50), a matrix name or a `ScoringMatrix`: what `Aligner`
    (``src/pyopal/lib.pyx:1202-1212``) and `pyopal.align` (``src/pyopal/_align.py:119-127``)
    accept; their error messages differ by one word."""
    if isinstance(spec, ScoringMatrix):
        return spec
    if spec is None:
        return Aligner._DEFAULT_SCORING_MATRIX
    if isinstance(spec, str):
        return ScoringMatrix.from_name(spec)
    raise TypeError(f"expected str or ScoringMatrix, {verb} {type(spec).__name__}")


class Aligner:
    """The Opal aligner, served by MI355X kernels
    (``src/pyopal/lib.pyx:1122-1383``)."""

    _DEFAULT_SCORING_MATRIX = ScoringMatrix.from_name("BLOSUM50")
    _DEFAULT_GAP_OPEN = 3
    _DEFAULT_GAP_EXTEND = 1

    def __init__(self, scoring_matrix=None, gap_open: int = _DEFAULT_GAP_OPEN,
                 gap_extend: int = _DEFAULT_GAP_EXTEND):
        self.scoring_matrix = resolve_scoring_matrix(scoring_matrix, "found")
        self.alphabet = Alphabet(self.scoring_matrix.alphabet)
        self.gap_open = int(gap_open)
        self.gap_extend = int(gap_extend)

        # the one backend: HIP kernels behind libmiopal.so (the slot where the
        # reference picks SSE2/SSE4/AVX2/NEON, src/pyopal/lib.pyx:1213-1227)
        try:
            _capi.lib()
        except (RuntimeError, OSError) as err:
            raise RuntimeError("no supported SIMD backend available") from err
        from .platform.hip import searchHIP
        self._search = searchHIP

        if not self.scoring_matrix.is_integer():
            raise ValueError("Integer scoring matrix is expected")
        self._int_matrix = self.scoring_matrix.int_array()
        self._matrix = _int_matrix_array(self._int_matrix)   # (as the device calls of the extensions take it)

    def __repr__(self):
        args = []
        if self.scoring_matrix != self._DEFAULT_SCORING_MATRIX:
            args.append(f"{self.scoring_matrix!r}")
        if self.gap_open != self._DEFAULT_GAP_OPEN:
            args.append(f"gap_open={self.gap_open!r}")
        if self.gap_extend != self._DEFAULT_GAP_EXTEND:
            args.append(f"gap_extend={self.gap_extend!r}")
        return f"{type(self).__name__}({', '.join(args)})"

    def __reduce__(self):
        return type(self), (self.scoring_matrix, self.gap_open, self.gap_extend)

    def __eq__(self, other):
        if not isinstance(other, Aligner):
            return NotImplemented
        return self.__reduce__()[1] == other.__reduce__()[1]

    __hash__ = None

    def align(self, query, database: BaseDatabase, *, mode: str = "score",
              overflow: str = "buckets", algorithm: str = "sw", start: int = 0,
              end: int = UINT32_MAX, device: int = 0,
              shard: typing.Optional[typing.Tuple[int, int]] = None,
              shard_version: typing.Optional[int] = None) -> typing.List[ScoreResult]:
        """Align the query to every target of ``database[start:end]``.

        Same keywords as the reference (``src/pyopal/lib.pyx:1258-1268``);
        ``device`` (extension) selects the GPU holding the database mirror, ``shard`` (extension)
        a mirror of the targets ``[lo, hi)`` only, which must contain ``[start, end)``: what
        `pyopal_amd.align` uses to give every GPU its own part of the database; with
        ``shard_version`` the shard only counts while the database is still in the state it was cut
        in (a database mutated since is searched through the whole-database mirror of ``device``).
        Target indices of the results are absolute either way.
        ``overflow`` is validated and otherwise ignored: the GPU path picks the
        narrowest exact lane width per target, results are identical.
        """
        if query is None:
            raise TypeError("Argument 'query' must not be None")
        if not isinstance(database, BaseDatabase):
            raise TypeError(f"Argument 'database' has incorrect type (expected BaseDatabase, "
                            f"got {type(database).__name__})")
        if mode in _OPAL_SEARCH_MODES:
            _mode = _OPAL_SEARCH_MODES[mode]
        else:
            raise ValueError(f"invalid search mode: {mode!r}")
        if overflow in _OPAL_OVERFLOW_MODES:
            _overflow = _OPAL_OVERFLOW_MODES[overflow]
        else:
            raise ValueError(f"invalid overflow mode: {overflow!r}")
        if algorithm in _OPAL_ALGORITHMS:
            _algo = _OPAL_ALGORITHMS[algorithm]
        else:
            raise ValueError(f"invalid algorithm: {algorithm!r}")
        if start < 0 or end < 0:
            raise OverflowError("can't convert negative value to uint32_t")

        if database.alphabet != self.alphabet:
            raise ValueError("database and score matrix have different alphabets")

        encoded = database.alphabet.encode(query)

        with database.lock.read:
            size = database._get_size()
            if shard is not None and shard_version is not None and getattr(database, "_version", None) != shard_version:
                shard = None
            if end < start:
                raise IndexError("database slice end is lower than start")
            if end > size:
                end = size
            if start > size:
                # the reference does not guard this case (unsigned underflow at
                # src/pyopal/platform/pyx.in:62); an IndexError is raised instead
                raise IndexError("database slice start is past the end of the database")
            if shard is not None and not (shard[0] <= start and end <= shard[1]):
                raise IndexError(f"slice [{start}, {end}) outside the shard [{shard[0]}, {shard[1]})")
            return self._search(encoded, database, _mode, _overflow, _algo, self.gap_open,
                                self.gap_extend, self._int_matrix, start, end, device=device, shard=shard)


    def scores(self, query, database: BaseDatabase, *, algorithm: str = "sw", start: int = 0,
               end: int = UINT32_MAX, device: int = 0) -> np.ndarray:
        """Extension: the scores of ``align(mode="score")`` as
        one ``int32`` array instead of a list of `ScoreResult` objects, which for a
        million targets costs more wall time than the search itself."""
        return self.align_arrays(query, database, mode="score", algorithm=algorithm, start=start,
                                 end=end, device=device).score

    def align_arrays(self, query, database: BaseDatabase, *, mode: str = "score",
                     algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX,
                     device: int = 0) -> "ResultArrays":
        """Extension: the results of `align` as arrays, one entry
        per target of ``database[start:end]``, without a Python object per target. The
        returned `ResultArrays` builds the reference's result objects on demand
        (``arrays[k]``, iteration), so ``list(arrays) == aligner.align(...)``."""
        return self._search_arrays(_Sequences(self, query, False), database, mode, algorithm, start, end, device)

    def _search_arrays(self, side: _QuerySide, database, mode, algorithm, start, end, device) -> "ResultArrays":
        """`align_arrays` / `align_pssm_arrays`: one search of the slice with one query or PSSM"""
        with _Request(side, database, mode, algorithm, start, end, device) as request:
            if request.end == request.start:
                return ResultArrays(mode, start, side.lengths[0], [], _empty_arrays(mode))
            mirror = request.mirror()
            out = side.search(mirror, mode, algorithm, start, request.end)
            lengths = np.diff(mirror.offsets[start:request.end + 1]) if mode == "full" else None
            return ResultArrays(mode, start, side.lengths[0], lengths, out)

    def align_pssm(self, pssm: "Pssm", database: BaseDatabase, *, mode: str = "score", algorithm: str = "sw",
                   start: int = 0, end: int = UINT32_MAX, device: int = 0) -> typing.List[ScoreResult]:
        """Extension: `align` with a position-specific scoring matrix (`Pssm`) in the place of the query and the
        aligner's matrix: ``pssm.scores[i, t]`` scores query position ``i`` against target residue ``t``. The gap
        penalties are the aligner's; its scoring matrix is not used. Same result objects as `align`
        (``FullResult.query_length`` is ``len(pssm)``; a position is a match where the target residue is the
        consensus'). ``align_pssm(Pssm.from_sequence(q, matrix), db)`` equals ``Aligner(matrix).align(q, db)``."""
        arrays = self.align_pssm_arrays(pssm, database, mode=mode, algorithm=algorithm, start=start, end=end,
                                        device=device)
        if len(arrays) == 0:
            return []
        from . import _results
        scores = np.ascontiguousarray(arrays.score, dtype=np.int32)
        if mode == "score":
            return _results.score_results(arrays.start, scores)
        if mode == "end":
            return _results.end_results(arrays.start, scores, arrays.query_end, arrays.target_end)
        with database.lock.read:
            lengths = database._get_lengths()
        return _results.full_results(arrays.start, scores, arrays.query_end, arrays.target_end, arrays.query_start,
                                     arrays.target_start, len(pssm), lengths, arrays.operations,
                                     arrays.operation_offsets)

    def align_pssm_arrays(self, pssm: "Pssm", database: BaseDatabase, *, mode: str = "score", algorithm: str = "sw",
                          start: int = 0, end: int = UINT32_MAX, device: int = 0) -> "ResultArrays":
        """`align_pssm` with the results as arrays (`ResultArrays`, as `align_arrays` returns them)."""
        return self._search_arrays(_Profiles(self, pssm, False), database, mode, algorithm, start, end, device)

    def align_many(self, queries, database: BaseDatabase, *, mode: str = "score", algorithm: str = "sw",
                   start: int = 0, end: int = UINT32_MAX, device: int = 0) -> typing.List[typing.List[ScoreResult]]:
        """Extension: align every query of ``queries`` to every target of ``database[start:end]``.

        Returns ``[aligner.align(q, database, mode=mode, ...) for q in queries]``, computed by one batched
        search for the modes ``score`` and ``end`` (queries of up to 64 residues share the GPU's launches;
        longer ones take the single-query path inside the same call). ``mode="full"`` is accepted and runs
        query by query through `align`. This is the batch form of the reference README's thread-pool loop.
        """
        if mode == "full":
            return [self.align(q, database, mode=mode, algorithm=algorithm, start=start, end=end, device=device)
                    for q in list(queries)]
        arrays = self.align_many_arrays(queries, database, mode=mode, algorithm=algorithm, start=start, end=end,
                                        device=device)
        return [list(arrays[i]) for i in range(len(arrays))]

    def align_many_arrays(self, queries, database: BaseDatabase, *, mode: str = "score", algorithm: str = "sw",
                          start: int = 0, end: int = UINT32_MAX, device: int = 0) -> "BatchResultArrays":
        """Extension: `align_arrays` of many queries in one batched search. Returns a `BatchResultArrays`
        whose ``score`` (and for ``mode="end"`` ``query_end`` / ``target_end``) are ``int32`` arrays of shape
        ``(len(queries), n)``; ``arrays[i]`` is the `ResultArrays` of query ``i``, equal to
        ``align_arrays(queries[i], ...)``. Modes ``score`` and ``end``."""
        if mode == "full":
            raise ValueError("align_many_arrays computes scores and end locations only (mode 'score' or 'end')")
        side = _Sequences(self, queries, True)
        with _Request(side, database, mode, algorithm, start, end, device) as request:
            n = request.end - start
            if n == 0 or not side.lengths:
                out = _empty_arrays(mode, (len(side.lengths), n))
            else:
                out = side.search(request.mirror(), mode, algorithm, start, request.end)
            return BatchResultArrays(mode, start, side.lengths, out)

    def align_pairs(self, queries, database: BaseDatabase, pairs, *, mode: str = "score", algorithm: str = "sw",
                    device: int = 0) -> typing.List[ScoreResult]:
        """Extension: align a list of (query, target) pairs in one call (include/miopal.h, miopalAlignPairs).

        ``pairs`` is a sequence of ``(query_index, target_index)`` or an ``(n, 2)`` integer array: indices into
        ``queries`` and into the database, in any order, repeats allowed. Returns one `ScoreResult` / `EndResult` /
        `FullResult` per pair, in pair order, each equal to
        ``self.align(queries[i], database, mode=mode, algorithm=algorithm, start=j, end=j + 1)[0]``: the hits of
        `top_hits_many`, the survivors of a prefilter, the candidate pairs of a clustering step."""
        return self._pair_list(_Sequences(self, queries, True), database, pairs, mode, algorithm, device)

    def _pair_list(self, side: _QuerySide, database, pairs, mode, algorithm, device) -> typing.List[ScoreResult]:
        """`align_pairs` / `align_pairs_pssm`: one pair-list call, its arrays as result objects in pair order"""
        request = _Request(side, database, mode, algorithm, device=device)
        pairs = np.asarray(pairs if len(pairs) else np.zeros((0, 2), dtype=np.int64))
        if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
            raise ValueError(f"pairs must be a sequence of ({side.pair_index}, target_index) integers")
        pairs = pairs.astype(np.int64, copy=False)
        with request:
            if len(pairs) == 0:
                return []
            if pairs[:, 0].min() < 0 or pairs[:, 0].max() >= len(side.lengths):
                raise IndexError(side.pair_outside)
            if pairs[:, 1].min() < 0 or pairs[:, 1].max() >= request.size:
                raise IndexError("target index of a pair outside the database")
            mirror = request.mirror()
            out = side.align_pairs(mirror, pairs[:, 0], pairs[:, 1], mode, algorithm)
            return _result_objects(mode, pairs[:, 1], pairs[:, 0], side.lengths, _target_lengths(mirror, mode), out)

    def _aligned(self, side: _QuerySide, mirror, pair_query, pair_target, algorithm,
                 **carry) -> typing.Dict[str, typing.Any]:
        """The "full" step behind a selection made on scores: the chosen (query, target) pairs in ONE pair-list call.
        Returns its arrays - without "aln", the per-pair views - and what the selection ``carry`` over beside them."""
        if len(pair_target):
            out = side.align_pairs(mirror, pair_query, pair_target, "full", algorithm)
            out.pop("aln", None)
        else:
            out = _empty_arrays("full")
        out.update(carry)
        return out

    def align_pairs_pssm(self, pssms, database: BaseDatabase, pairs, *, mode: str = "score", algorithm: str = "sw",
                         device: int = 0) -> typing.List[ScoreResult]:
        """Extension: `align_pairs` with a list of `Pssm` in the place of the queries (include/miopal.h,
        miopalAlignPairsPssm): ``pairs`` holds ``(pssm_index, target_index)``. Returns one result per pair, in pair
        order, each equal to ``self.align_pssm(pssms[i], database, mode=mode, algorithm=algorithm, start=j,
        end=j + 1)[0]`` (``FullResult.query_length`` is ``len(pssms[i])``): a library of PSSMs against the
        survivors of a prefilter, the hits of a family scan. The gap penalties are the aligner's."""
        return self._pair_list(_Profiles(self, pssms, True), database, pairs, mode, algorithm, device)

    def profile_columns(self, query, database: BaseDatabase, targets, *, algorithm: str = "sw", return_msa: bool = False,
                        device: int = 0) -> "ProfileColumns":
        """Extension: the query-anchored profile columns of ``query`` and the targets ``targets`` (include/miopal.h,
        miopalProfileColumns) - the step between two rounds of an iterated profile search. ``query``: a sequence, or a
        `Pssm` (the aligner's matrix is then not used); ``targets``: a sequence or array of integer target indices, any
        order, repeats allowed - ``[h.target_index for h in hits]``. Every target is aligned as
        ``align_pairs(..., mode="full")`` aligns it, the alignments are projected onto the query's positions, and the
        letters per position are counted and weighted (Henikoff position-based weights) on the GPU in integers: only
        the columns and one weight per member come back. Returns a `ProfileColumns`; ``return_msa=True`` also brings
        the multiple alignment. An empty ``targets`` is the profile of the query alone and needs no device."""
        side = (_Profiles if isinstance(query, Pssm) else _Sequences)(self, query, False)
        request = _Request(side, database, None, algorithm, device=device)
        targets = np.asarray(targets if len(targets) else np.zeros(0, dtype=np.int64))
        if targets.ndim != 1 or not np.issubdtype(targets.dtype, np.integer):
            raise ValueError("targets must be a sequence of integer target indices")
        targets = targets.astype(np.int64, copy=False)
        alphabet = database.alphabet
        with request:
            if len(targets) == 0:
                return ProfileColumns.of_query(side.codes, alphabet, return_msa)
            if targets.min() < 0 or targets.max() >= request.size:
                raise IndexError("target index outside the database")
            out = side.profile_columns(request.mirror(), targets, algorithm, return_msa)
        return ProfileColumns(out["counts"], out["weighted"], out["member_weights"], alphabet, side.codes, out["msa"])

    def iterated_search(self, query, database: BaseDatabase, max_evalue: float, *, rounds: int = 3, algorithm: str = "sw",
                        background=None, pseudocount: float = 10.0, exclude_z: float = 5.0, device: int = 0):
        """Extension: an iterated profile search composed of the public steps. Round 1 is ``significant_hits(query)``;
        every further round builds the next `Pssm` from the hits of the one before - `profile_columns` with the round's
        query and its hit indices, then `Pssm.from_columns` with `matrix_lambda` of the aligner's matrix - and searches
        with `significant_hits_pssm`. It stops when the set of hit indices repeats or after ``rounds`` searches.
        ``background``: one frequency per letter; None: the residue composition of the database's sequences. Returns
        ``(the SignificantHits of the last search, the last Pssm or None, the hit-index arrays of every round)``."""
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)):
            raise TypeError(f"rounds must be an integer, not {type(rounds).__name__}")
        if rounds < 1:
            raise ValueError(f"rounds must be at least 1, got {rounds}")
        kw = dict(algorithm=algorithm, exclude_z=exclude_z, device=device)
        hits = self.significant_hits(query, database, max_evalue, **kw)
        found = [np.array(sorted(h.target_index for h in hits.results), dtype=np.int64)]
        if rounds == 1:
            return hits, None, found
        if background is None:
            with database.lock.read:
                residues = np.frombuffer(b"".join(database._get_encoded()), dtype=np.uint8)
            background = np.bincount(residues, minlength=len(self.alphabet))[:len(self.alphabet)].astype(np.float64)
        background = np.asarray(background, dtype=np.float64) / np.sum(background)
        lam = matrix_lambda(self.scoring_matrix, background)
        current, pssm = query, None
        prior = Pssm.from_sequence(query, self.scoring_matrix)
        while len(found) < rounds:
            columns = self.profile_columns(current, database, found[-1], algorithm=algorithm, device=device)
            pssm = Pssm.from_columns(columns, prior, background, lam, pseudocount=pseudocount)
            hits = self.significant_hits_pssm(pssm, database, max_evalue, **kw)
            found.append(np.array(sorted(h.target_index for h in hits.results), dtype=np.int64))
            if any(np.array_equal(found[-1], earlier) for earlier in found[:-1]):
                break
            current = prior = pssm
        return hits, pssm, found

    def top_hits_pssm(self, pssm: "Pssm", database: BaseDatabase, k: int = 10, *, mode: str = "score",
                      algorithm: str = "sw", min_score: typing.Optional[int] = None, start: int = 0,
                      end: int = UINT32_MAX, device: int = 0) -> typing.List[ScoreResult]:
        """Extension: `top_hits` with a `Pssm` in the place of the query and the aligner's matrix
        (include/miopal.h, miopalSearchPssmTop): the ``k`` best targets of ``database[start:end]``, best first,
        selected on the GPU. Equal to ``[r for r in sorted(self.align_pssm(pssm, database, mode=mode, ...),
        key=lambda r: r.score, reverse=True) if min_score is None or r.score >= min_score][:k]``. ``mode="full"``
        selects on the scores, then aligns the chosen targets only, in one pair-list call (miopalAlignPairsPssm):
        the step an iterated profile search repeats."""
        return self._top(_Profiles(self, pssm, False), database, k, mode, algorithm, min_score, start, end, device)[0]

    def top_hits(self, query, database: BaseDatabase, k: int = 10, *, mode: str = "score", algorithm: str = "sw",
                 min_score: typing.Optional[int] = None, start: int = 0, end: int = UINT32_MAX,
                 device: int = 0) -> typing.List[ScoreResult]:
        """Extension: the ``k`` best targets of ``database[start:end]``, best first, selected on the GPU
        (include/miopal.h, miopalSearchTop): only ``k`` entries leave the device. Equal to
        ``[r for r in sorted(self.align(query, database, mode=mode, ...), key=lambda r: r.score, reverse=True)
        if min_score is None or r.score >= min_score][:k]``. ``mode="full"`` selects on the scores, then aligns the
        chosen targets only, in one pair-list call (miopalAlignPairs)."""
        return self._top(_Sequences(self, query, False), database, k, mode, algorithm, min_score, start, end, device)[0]

    def top_hits_many(self, queries, database: BaseDatabase, k: int = 10, *, mode: str = "score",
                      algorithm: str = "sw", min_score: typing.Optional[int] = None, start: int = 0,
                      end: int = UINT32_MAX, device: int = 0) -> typing.List[typing.List[ScoreResult]]:
        """Extension: `top_hits` of every query of ``queries`` in one batched search
        (miopalSearchBatchTop); returns one list per query. ``mode="full"`` selects on the scores, then aligns
        all chosen (query, target) pairs in ONE pair-list call (miopalAlignPairs)."""
        return self._top(_Sequences(self, queries, True), database, k, mode, algorithm, min_score, start, end, device)

    def _top(self, side: _QuerySide, database, k, mode, algorithm, min_score, start, end, device):
        """`top_hits` and its forms: one list of result objects per query of ``side``, the device selection on the scores
        (and end locations), and for "full" the chosen pairs aligned behind it."""
        if min_score is not None:
            min_score = int(min_score)
        with _Request(side, database, mode, algorithm, start, end, device,
                      lambda: _count_argument("k", k, 0, _capi.MIOPAL_MAX_TOP, "MIOPAL_MAX_TOP")) as request:
            k = request.checked
            if request.end == start or k == 0 or not side.lengths:
                return [[] for _ in side.lengths]
            mirror = request.mirror()
            counts, out = side.top(mirror, "score" if mode == "full" else mode, algorithm, start, request.end, k,
                                   min_score)
            rows = [{key: table[i, :c] for key, table in out.items()} for i, c in enumerate(counts)]
            if mode != "full":
                return [_result_objects(mode, row["target"], None, None, None, row) for row in rows]
            target = np.concatenate([row["target"] for row in rows])
            owner = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
            arrays = self._aligned(side, mirror, owner, target, algorithm)
            return _cut(_result_objects(mode, target, owner, side.lengths, _target_lengths(mirror, mode), arrays), counts)

    def best_queries(self, queries, database: BaseDatabase, m: int = 1, *, mode: str = "score", algorithm: str = "sw",
                     min_score: typing.Optional[int] = None, start: int = 0, end: int = UINT32_MAX,
                     device: int = 0) -> typing.List[typing.List[typing.Tuple[int, ScoreResult]]]:
        """Extension: the ``m`` best queries of every target of ``database[start:end]``, selected on the GPU
        (include/miopal.h, miopalSearchBatchTargetTop): which barcode, adapter or motif of ``queries`` matches each
        read best, and the runner-up for the margin. Returns one list per target of ``(query_index, result)``, best
        first (score descending, query index ascending), at most ``m`` long; ``result`` equals
        ``self.align(queries[query_index], database, mode=mode, ...)[target]``. ``min_score``: only queries scoring at
        least that many count. ``mode="full"`` selects on the scores, then aligns all chosen (query, target) pairs in
        ONE pair-list call (miopalAlignPairs)."""
        out, side, mirror = self._best_queries(queries, database, m, mode, algorithm, min_score, start, end, device)
        counts = out.pop("count")
        chosen = np.arange(out["query"].shape[1])[None, :] < counts[:, None]
        target = np.repeat(np.arange(start, start + len(counts), dtype=np.int64), counts)
        arrays = out["pairs"] if mode == "full" else {key: table[chosen] for key, table in out.items()}
        index = out["query"][chosen].tolist()
        flat = _result_objects(mode, target, index, side.lengths, _target_lengths(mirror, mode), arrays)
        return _cut(list(zip(index, flat)), counts.tolist())

    def best_queries_arrays(self, queries, database: BaseDatabase, m: int = 1, *, mode: str = "score",
                            algorithm: str = "sw", min_score: typing.Optional[int] = None, start: int = 0,
                            end: int = UINT32_MAX, device: int = 0) -> typing.Dict[str, typing.Any]:
        """`best_queries` without result objects: "count" (one per target), and "query" (int32), "score" - for "end"
        also "end_q" / "end_t" - of shape (targets, m), best first, -1 past the count. For "full" also "pairs": the
        arrays of the one `align_pairs` call on all chosen pairs - "query", "target", "score", "end_q" / "end_t",
        "start_q" / "start_t", "aln_flat" / "aln_off" - row-major over (target, rank) for rank < count."""
        return self._best_queries(queries, database, m, mode, algorithm, min_score, start, end, device)[0]

    def _best_queries(self, queries, database, m, mode, algorithm, min_score, start, end, device):
        """The arrays of `best_queries_arrays`, the query side and the device mirror (None where none was needed): the
        device selection, and for "full" the chosen pairs aligned behind it, row-major over (target, rank)."""
        if min_score is not None:
            min_score = int(min_score)
        side = _Sequences(self, queries, True)
        with _Request(side, database, mode, algorithm, start, end, device,
                      lambda: _count_argument("m", m, 1, _capi.MIOPAL_MAX_TARGET_TOP, "MIOPAL_MAX_TARGET_TOP")) as request:
            m = request.checked
            n = request.end - start
            search_mode = "score" if mode == "full" else mode
            if n == 0 or not side.lengths:
                mirror = None
                out = dict(_empty_arrays(search_mode, (n, m), -1), count=np.zeros(n, dtype=np.int32),
                           query=np.full((n, m), -1, dtype=np.int32))
            else:
                mirror = request.mirror()
                out = mirror.search_batch_target_top(side.arrays, self._matrix, self.gap_open, self.gap_extend,
                                                     search_mode, algorithm, start, request.end, m, min_score)
            if mode == "full":
                pair_query = out["query"][np.arange(m)[None, :] < out["count"][:, None]]
                pair_target = np.repeat(np.arange(start, request.end, dtype=np.int64), out["count"])
                out["pairs"] = self._aligned(side, mirror, pair_query, pair_target, algorithm, query=pair_query,
                                             target=pair_target)
            return out, side, mirror

    def hits(self, query, database: BaseDatabase, min_score: int, *, mode: str = "score", algorithm: str = "sw",
             start: int = 0, end: int = UINT32_MAX, device: int = 0, max_hits: typing.Optional[int] = None,
             sort: bool = False) -> typing.List[ScoreResult]:
        """Extension: every target of ``database[start:end]`` that scores at least ``min_score``, compacted on the
        GPU (include/miopal.h, miopalSearchHits): only the hits leave the device, however many there are (`top_hits`
        stops at 4096). Equal to ``[r for r in self.align(query, database, mode=mode, ...) if r.score >= min_score]``,
        in database order; ``sort=True`` orders best first (score descending, index ascending: `top_hits`' order) on
        the host. ``mode="full"`` selects on the scores, then aligns the hits only, in one pair-list call
        (miopalAlignPairs). With more than ``max_hits`` hits: `_capi.TooManyHits`, its ``counts`` the number."""
        arrays = self._hit_arrays(_Sequences(self, query, False), database, min_score, mode, algorithm, start, end, device,
                                  max_hits, sort)
        return self._hit_objects(*arrays, mode)[0]

    def hits_arrays(self, query, database: BaseDatabase, min_score: int, *, mode: str = "score", algorithm: str = "sw",
                    start: int = 0, end: int = UINT32_MAX, device: int = 0, max_hits: typing.Optional[int] = None,
                    sort: bool = False) -> typing.Dict[str, np.ndarray]:
        """`hits` without result objects: "target" (int64) and "score" - for "end" and "full" also "end_q" / "end_t",
        for "full" also "start_q" / "start_t", "aln_flat" / "aln_off" - one entry per hit (and "offsets": [0, hits])."""
        arrays = self._hit_arrays(_Sequences(self, query, False), database, min_score, mode, algorithm, start, end, device,
                                  max_hits, sort)
        return arrays[0]

    def hits_many(self, queries, database: BaseDatabase, min_score, *, mode: str = "score", algorithm: str = "sw",
                  start: int = 0, end: int = UINT32_MAX, device: int = 0, max_hits: typing.Optional[int] = None,
                  sort: bool = False) -> typing.List[typing.List[ScoreResult]]:
        """Extension: `hits` of every query of ``queries`` in one batched search (miopalSearchBatchHits); returns one
        list per query. ``min_score``: an integer, or one per query. ``max_hits`` bounds the total over all queries.
        ``mode="full"`` aligns all (query, hit) pairs in ONE pair-list call."""
        arrays = self._hit_arrays(_Sequences(self, queries, True), database, min_score, mode, algorithm, start, end, device,
                                  max_hits, sort)
        return self._hit_objects(*arrays, mode)

    def hits_many_arrays(self, queries, database: BaseDatabase, min_score, *, mode: str = "score",
                         algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                         max_hits: typing.Optional[int] = None, sort: bool = False) -> typing.Dict[str, np.ndarray]:
        """`hits_many` as a CSR, for callers that want no objects (the edge list of an all-against-all comparison):
        "offsets" (len(queries) + 1,), and `hits_arrays`' arrays with entries offsets[i]:offsets[i + 1] the hits of
        query i."""
        arrays = self._hit_arrays(_Sequences(self, queries, True), database, min_score, mode, algorithm, start, end, device,
                                  max_hits, sort)
        return arrays[0]

    def hits_pssm(self, pssm: "Pssm", database: BaseDatabase, min_score: int, *, mode: str = "score",
                  algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                  max_hits: typing.Optional[int] = None, sort: bool = False) -> typing.List[ScoreResult]:
        """Extension: `hits` with a `Pssm` in the place of the query and the aligner's matrix (miopalSearchPssmHits):
        equal to ``[r for r in self.align_pssm(pssm, database, mode=mode, ...) if r.score >= min_score]``.
        ``mode="full"`` aligns the hits in one pair-list call (miopalAlignPairsPssm): all targets above the inclusion
        threshold, the step an iterated profile search repeats."""
        arrays = self._hit_arrays(_Profiles(self, pssm, False), database, min_score, mode, algorithm, start, end, device,
                                  max_hits, sort)
        return self._hit_objects(*arrays, mode)[0]

    def hits_pssm_arrays(self, pssm: "Pssm", database: BaseDatabase, min_score: int, *, mode: str = "score",
                         algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                         max_hits: typing.Optional[int] = None, sort: bool = False) -> typing.Dict[str, np.ndarray]:
        """`hits_pssm` without result objects (`hits_arrays`' dict)."""
        arrays = self._hit_arrays(_Profiles(self, pssm, False), database, min_score, mode, algorithm, start, end, device,
                                  max_hits, sort)
        return arrays[0]

    @staticmethod
    def _hit_thresholds(min_score, count, many):
        """``min_score`` as one int32 per query: an integer, or (hits_many) a sequence of ``count`` integers."""
        per_query = many and not isinstance(min_score, (int, np.integer, str)) and np.ndim(min_score) == 1
        values = list(min_score) if per_query else [min_score]
        for v in values:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"min_score must be an integer, not {type(v).__name__}")
            if not -(2 ** 31) <= int(v) < 2 ** 31:
                raise OverflowError("min_score does not fit a 32-bit integer")
        if per_query and len(values) != count:
            raise ValueError(f"min_score must be an integer or hold one per query ({count}), got {len(values)}")
        return np.array([int(v) for v in values] if per_query else [int(min_score)] * count, dtype=np.int32)

    @staticmethod
    def _evalue_cuts(max_evalue, count, many):
        """``max_evalue`` as one float64 per query: a finite positive number, or (significant_hits_many) a sequence
        of ``count`` of them."""
        per_query = many and not isinstance(max_evalue, (int, float, np.number, str)) and np.ndim(max_evalue) == 1
        values = list(max_evalue) if per_query else [max_evalue]
        for v in values:
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise TypeError(f"max_evalue must be a number, not {type(v).__name__}")
            if not np.isfinite(v) or not v > 0:
                raise ValueError("max_evalue must be finite and positive")
        if per_query and len(values) != count:
            raise ValueError(f"max_evalue must be a number or hold one per query ({count}), got {len(values)}")
        return np.array([float(v) for v in values] if per_query else [float(max_evalue)] * count, dtype=np.float64)

    @staticmethod
    def _exclude_z(exclude_z):
        if isinstance(exclude_z, bool) or not isinstance(exclude_z, (int, float, np.integer, np.floating)):
            raise TypeError(f"exclude_z must be a number, not {type(exclude_z).__name__}")
        if np.isnan(exclude_z):
            raise ValueError("exclude_z must not be NaN")
        return float(exclude_z)

    def _hit_arrays(self, side: _QuerySide, database, min_score, mode, algorithm, start, end, device, max_hits, sort,
                    significant=None):
        """The CSR of `hits` and its forms: the device selection, the host sort, and for "full" the hits aligned behind
        them. Returns (arrays, (query lengths, target lengths or None)): what `_hit_objects` needs beside the arrays.
        ``significant``: (max_evalue, exclude_z) of the `significant_hits` forms in the place of ``min_score`` - the
        arrays then hold "evalue", "zscore" and "fits" (one `ScoreFit` per query) as well, and ``sort`` orders by
        E-value, then index."""
        request = _Request(side, database, mode, algorithm, start, end, device, lambda: _max_hits_argument(max_hits))
        max_hits, count = request.checked, len(side.lengths)
        if significant is None:
            thresholds = self._hit_thresholds(min_score, count, side.many)
        else:
            cuts, exclude_z = self._evalue_cuts(significant[0], count, side.many), self._exclude_z(significant[1])
        with request:
            if request.end == start or count == 0:
                out = dict(_empty_arrays(mode), offsets=np.zeros(count + 1, dtype=np.int64),
                           target=np.zeros(0, dtype=np.int64))
                if significant is not None:
                    out.update(evalue=np.zeros(0, dtype=np.float64), zscore=np.zeros(0, dtype=np.float64),
                               fits=[ScoreFit() for _ in range(count)])
                return out, (side.lengths, None)
            mirror = request.mirror()
            search_mode = "score" if mode == "full" else mode
            if significant is None:
                got = side.hits(mirror, search_mode, algorithm, start, request.end, thresholds, max_hits)
            else:
                got = side.significant(mirror, search_mode, algorithm, start, request.end, cuts, exclude_z, max_hits)
            offsets = got["offsets"]
            owner = np.repeat(np.arange(count, dtype=np.int32), np.diff(offsets))
            if sort and len(owner):
                # best first inside every query: score descending, then index ascending (`top_hits`' order); the
                # significant forms: E-value ascending, then index
                first = got["evalue"] if significant is not None else -got["score"].astype(np.int64)
                order = np.lexsort((got["target"], first, owner))
                for key in ("target", "score", "end_q", "end_t", "evalue"):
                    if key in got:
                        got[key] = got[key][order]
            if significant is not None:
                lengths = np.diff(mirror.offsets)[got["target"]]
                got["zscore"] = np.zeros(len(owner), dtype=np.float64)
                for i, fit in enumerate(got["fits"]):
                    span = slice(int(offsets[i]), int(offsets[i + 1]))
                    got["zscore"][span] = fit.zscore(got["score"][span], lengths[span])
            if mode == "full":
                # every (query, hit) pair, in the order chosen above
                carry = {key: got[key] for key in ("offsets", "target", "evalue", "zscore", "fits") if key in got}
                got = self._aligned(side, mirror, owner, got["target"], algorithm, **carry)
            return got, (side.lengths, _target_lengths(mirror, mode))

    def _significant_objects(self, out, lengths, mode):
        offsets = out["offsets"].tolist()
        return [SignificantHits(results, out["evalue"][offsets[i]:offsets[i + 1]], out["zscore"][offsets[i]:offsets[i + 1]],
                                out["fits"][i])
                for i, results in enumerate(self._hit_objects(out, lengths, mode))]

    @staticmethod
    def _hit_objects(out, lengths, mode):
        """The CSR of `_hit_arrays` as one list of result objects per query."""
        counts = np.diff(out["offsets"])
        owner = np.repeat(np.arange(len(counts)), counts) if mode == "full" else None
        return _cut(_result_objects(mode, out["target"], owner, lengths[0], lengths[1], out), counts.tolist())

    def significant_hits(self, query, database: BaseDatabase, max_evalue: float, *, mode: str = "score",
                         algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                         exclude_z: float = 5.0, max_hits: typing.Optional[int] = None,
                         sort: bool = False) -> "SignificantHits":
        """Extension: every target of ``database[start:end]`` with an E-value of at most ``max_evalue`` (include/miopal.h,
        miopalSearchSignificant) - `hits` with the cut stated the way a search states it, "include below 1e-3". The
        search is its own calibration sample: the scores are regressed on ln(target length) per quarter-octave length
        bin, from integer sums gathered on the GPU, standardised, and the z-scores read against the extreme-value
        distribution; the cut becomes one integer threshold per length bin and the hits are compacted on the GPU.
        ``exclude_z``: targets more than that many standard deviations above the line are left out of the fit (up to
        three refits; 0: one pass). Returns a `SignificantHits`: ``.results`` (what `hits` returns, database order),
        ``.evalues`` / ``.zscores`` (float64) and ``.fit`` (a `ScoreFit`); iterating yields (result, evalue).
        ``sort=True``: E-value ascending, then index. ``mode="full"`` aligns the hits in one pair-list call. The
        z-score holds for any algorithm; the E-value is calibrated for local ("sw") scores."""
        arrays = self._hit_arrays(_Sequences(self, query, False), database, None, mode, algorithm, start, end, device,
                                  max_hits, sort, (max_evalue, exclude_z))
        return self._significant_objects(*arrays, mode)[0]

    def significant_hits_arrays(self, query, database: BaseDatabase, max_evalue: float, *, mode: str = "score",
                                algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                                exclude_z: float = 5.0, max_hits: typing.Optional[int] = None,
                                sort: bool = False) -> typing.Dict[str, typing.Any]:
        """`significant_hits` without result objects: `hits_arrays`' dict plus "evalue", "zscore" and "fit"."""
        arrays = self._hit_arrays(_Sequences(self, query, False), database, None, mode, algorithm, start, end, device,
                                  max_hits, sort, (max_evalue, exclude_z))
        arrays[0]["fit"] = arrays[0].pop("fits")[0]
        return arrays[0]

    def significant_hits_many(self, queries, database: BaseDatabase, max_evalue, *, mode: str = "score",
                              algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                              exclude_z: float = 5.0, max_hits: typing.Optional[int] = None,
                              sort: bool = False) -> typing.List["SignificantHits"]:
        """Extension: `significant_hits` of every query in one batched search (miopalSearchBatchSignificant); one
        `SignificantHits` per query. ``max_evalue``: a number, or one per query."""
        arrays = self._hit_arrays(_Sequences(self, queries, True), database, None, mode, algorithm, start, end, device,
                                  max_hits, sort, (max_evalue, exclude_z))
        return self._significant_objects(*arrays, mode)

    def significant_hits_many_arrays(self, queries, database: BaseDatabase, max_evalue, *, mode: str = "score",
                                     algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                                     exclude_z: float = 5.0, max_hits: typing.Optional[int] = None,
                                     sort: bool = False) -> typing.Dict[str, typing.Any]:
        """`significant_hits_many` as `hits_many_arrays`' CSR plus "evalue", "zscore" and "fits" (one per query)."""
        arrays = self._hit_arrays(_Sequences(self, queries, True), database, None, mode, algorithm, start, end, device,
                                  max_hits, sort, (max_evalue, exclude_z))
        return arrays[0]

    def significant_hits_pssm(self, pssm: "Pssm", database: BaseDatabase, max_evalue: float, *, mode: str = "score",
                              algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX, device: int = 0,
                              exclude_z: float = 5.0, max_hits: typing.Optional[int] = None,
                              sort: bool = False) -> "SignificantHits":
        """Extension: `significant_hits` with a `Pssm` in the place of the query and the aligner's matrix
        (miopalSearchPssmSignificant): the inclusion step of an iterated profile search."""
        arrays = self._hit_arrays(_Profiles(self, pssm, False), database, None, mode, algorithm, start, end, device,
                                  max_hits, sort, (max_evalue, exclude_z))
        return self._significant_objects(*arrays, mode)[0]

    def significant_hits_pssm_arrays(self, pssm: "Pssm", database: BaseDatabase, max_evalue: float, *,
                                     mode: str = "score", algorithm: str = "sw", start: int = 0, end: int = UINT32_MAX,
                                     device: int = 0, exclude_z: float = 5.0, max_hits: typing.Optional[int] = None,
                                     sort: bool = False) -> typing.Dict[str, typing.Any]:
        """`significant_hits_pssm` without result objects (`significant_hits_arrays`' dict)."""
        arrays = self._hit_arrays(_Profiles(self, pssm, False), database, None, mode, algorithm, start, end, device,
                                  max_hits, sort, (max_evalue, exclude_z))
        arrays[0]["fit"] = arrays[0].pop("fits")[0]
        return arrays[0]


class ScoreFit:
    """The score statistics behind a `significant_hits` call (include/miopal.h, MiopalScoreFit): per quarter-octave
    length bin the integer sums gathered on the GPU, the line mean score = ``intercept`` + ``slope`` ln(length) with
    the spread ``sigma`` fitted to them, and the integer threshold per bin the E-value cut became. ``degenerate``: too
    few targets (or no spread) for a fit - nothing is a hit, z-scores and E-values are NaN."""

    def __init__(self, raw: typing.Optional[_capi.ScoreFit] = None):
        bins = _capi.MIOPAL_STAT_BINS
        if raw is None:
            raw = _capi.ScoreFit()
            raw.degenerate = 1
            for b in range(bins):
                raw.ceiling[b] = raw.threshold[b] = 2 ** 31 - 1
        self.targets, self.used, self.passes = int(raw.targets), int(raw.used), int(raw.passes)
        self.degenerate = bool(raw.degenerate)
        self.intercept, self.slope, self.sigma, self.z_cut = (float(raw.intercept), float(raw.slope), float(raw.sigma),
                                                              float(raw.zCut))
        self.bin_targets = np.array(raw.binTargets, dtype=np.int64)
        self.bin_length = np.array(raw.binLength, dtype=np.int64)
        self.all = np.array(raw.all, dtype=np.int64).reshape(bins, 3)
        self.kept = np.array(raw.kept, dtype=np.int64).reshape(bins, 3)
        self.ceilings = np.array(raw.ceiling, dtype=np.int32)
        self.thresholds = np.array(raw.threshold, dtype=np.int32)

    def bin_means(self) -> np.ndarray:
        """The line's mean score of every bin (NaN for bin 0 and bins that hold no targets)."""
        mean = np.full(_capi.MIOPAL_STAT_BINS, np.nan)
        held = self.bin_targets > 0
        held[0] = False
        if not self.degenerate:
            mean[held] = self.intercept + self.slope * np.log(self.bin_length[held] / self.bin_targets[held])
        return mean

    def zscore(self, score, length) -> np.ndarray:
        """(score - mean of the length's bin) / sigma, elementwise."""
        bins = _capi.length_bins(length)
        if self.degenerate:
            return np.full(np.broadcast(np.asarray(score), bins).shape, np.nan)
        return (np.asarray(score, dtype=np.float64) - self.bin_means()[bins]) / self.sigma

    def evalue(self, score, length) -> np.ndarray:
        """targets x P(z), P the upper tail of a Gumbel variable with mean 0 and variance 1."""
        z = self.zscore(score, length)
        return self.targets * -np.expm1(-np.exp(-(np.pi / np.sqrt(6.0)) * z - np.euler_gamma))

    def threshold(self, length) -> np.ndarray:
        """The smallest score that makes a target of that length a hit (2^31 - 1: never)."""
        return self.thresholds[_capi.length_bins(length)]

    def __repr__(self):
        return (f"ScoreFit(targets={self.targets}, used={self.used}, passes={self.passes}, intercept={self.intercept:.4g}, "
                f"slope={self.slope:.4g}, sigma={self.sigma:.4g}, z_cut={self.z_cut:.4g}, degenerate={self.degenerate})")


class SignificantHits:
    """What `Aligner.significant_hits` returns: ``results`` (the objects `Aligner.hits` returns), ``evalues`` and
    ``zscores`` (float64, the same order) and ``fit`` (a `ScoreFit`). Iterating yields (result, evalue)."""

    def __init__(self, results, evalues, zscores, fit):
        self.results, self.evalues, self.zscores, self.fit = results, evalues, zscores, fit

    def __len__(self):
        return len(self.results)

    def __iter__(self):
        return iter(zip(self.results, self.evalues.tolist()))

    def __repr__(self):
        return f"SignificantHits({len(self.results)} hits, {self.fit!r})"


class Pssm:
    """A position-specific scoring matrix: the query of `Aligner.align_pssm`.

    ``scores``: integers of shape ``(Q, len(alphabet))``, ``scores[i, t]`` the score of aligning position ``i`` with
    residue ``alphabet[t]``; kept as a contiguous, read-only ``int32`` array. ``alphabet``: an `Alphabet` or its
    letters (default: the protein alphabet). ``consensus``: the residue a position counts as when an alignment tells
    matches from mismatches - a string over the alphabet or ``Q`` residue codes (255: no residue, never a match);
    default: each row's best-scoring letter, the lowest index on ties. Kept as a read-only ``uint8`` array of
    codes; `consensus_sequence` is its text. `from_columns` builds the next round's PSSM from the `ProfileColumns`
    of a search's hits (position-based sequence weights, pseudocounts from the prior round, log-odds against a
    background). Still out of scope: per-column reduced alignments as PSI-BLAST weights them, composition-based
    statistics, insertion-aware profiles."""

    NO_RESIDUE = 255
    __slots__ = ("scores", "alphabet", "consensus")

    def __init__(self, scores, alphabet=None, consensus=None):
        if alphabet is None:
            alphabet = Alphabet()
        elif isinstance(alphabet, str):
            alphabet = Alphabet(alphabet)
        elif not isinstance(alphabet, Alphabet):
            raise TypeError(f"expected str or Alphabet, found {type(alphabet).__name__}")
        raw = np.asarray(scores)
        if raw.dtype == object or not (np.issubdtype(raw.dtype, np.integer) or
                                       (np.issubdtype(raw.dtype, np.floating) and np.all(raw == np.rint(raw)))):
            raise ValueError("Integer scores are expected")
        if raw.ndim != 2 or raw.shape[1] != len(alphabet):
            raise ValueError(f"scores must have shape (positions, {len(alphabet)}), found {raw.shape}")
        if raw.size and (raw.min() < -(2 ** 31) or raw.max() >= 2 ** 31):
            raise OverflowError("scores do not fit 32-bit integers")
        rows = np.array(raw, dtype=np.int32, order="C")
        rows.setflags(write=False)
        if consensus is None:
            codes = rows.argmax(axis=1).astype(np.uint8) if len(rows) else np.zeros(0, dtype=np.uint8)
        elif isinstance(consensus, str):
            codes = np.frombuffer(alphabet.encode(consensus), dtype=np.uint8).copy()
        else:
            wide = np.asarray(consensus)
            if wide.ndim != 1 or (wide.size and not np.issubdtype(wide.dtype, np.integer)):
                raise ValueError("consensus must be a string or a sequence of residue codes")
            if wide.size and np.any(((wide < 0) | (wide >= len(alphabet))) & (wide != self.NO_RESIDUE)):
                raise ValueError(f"consensus residues must be below {len(alphabet)}, or {self.NO_RESIDUE}")
            codes = wide.astype(np.uint8)
        if len(codes) != len(rows):
            raise ValueError(f"consensus has {len(codes)} residues for {len(rows)} positions")
        codes.setflags(write=False)
        self.scores = rows
        self.alphabet = alphabet
        self.consensus = codes

    @classmethod
    def from_sequence(cls, sequence, scoring_matrix="BLOSUM62") -> "Pssm":
        """The PSSM of an ordinary query: row ``i`` is the matrix row of ``sequence[i]``, the consensus the
        sequence itself. Searching with it gives what the sequence gives under that matrix."""
        matrix = resolve_scoring_matrix(scoring_matrix, "found")
        if not matrix.is_integer():
            raise ValueError("Integer scoring matrix is expected")
        alphabet = Alphabet(matrix.alphabet)
        codes = np.frombuffer(alphabet.encode(sequence), dtype=np.uint8)
        table = _int_matrix_array(matrix.int_array()).reshape(len(alphabet), len(alphabet))
        return cls(table[codes], alphabet, codes)

    def reverse_complement(self, complement=None) -> "Pssm":
        """The PSSM of the other strand: the rows in reverse order, their columns and the consensus permuted by
        ``complement``, a mapping over the alphabet's letters (letters it leaves out map to themselves). Default:
        A and T, C and G are exchanged, U is mapped like T where the alphabet has it, every other letter stays; an
        alphabet that holds none of these pairs raises ValueError, and so does one with a letter that is no IUPAC
        nucleotide code - the protein alphabet has A, C, G and T, and exchanging those amino acids without being asked
        to would be a wrong answer, not a default. ``NO_RESIDUE`` in the consensus stays. A motif
        library is scanned on both strands by putting each PSSM and its reverse complement into the panel
        (`find_occurrences_pssm_many`). Host-only."""
        letters = self.alphabet.letters
        if complement is None:
            pairs = [(a, b) for a, b in (("A", "T"), ("C", "G"), ("A", "U")) if a in letters and b in letters]
            if not pairs:
                raise ValueError("the alphabet holds none of the pairs A/T, C/G, A/U: pass a complement mapping")
            if any(x not in "ACGTUNRYSWKMBDHV*" for x in letters):
                raise ValueError("the alphabet holds letters that are no nucleotide codes: pass a complement mapping")
            complement = {}
            for a, b in pairs:
                complement[b] = a
                complement.setdefault(a, b)   # (A goes to T where both T and U stand)
        elif not isinstance(complement, typing.Mapping):
            raise TypeError(f"complement must be a mapping of letters, not {type(complement).__name__}")
        to = np.arange(len(letters), dtype=np.int64)
        for a, b in complement.items():
            if not (isinstance(a, str) and isinstance(b, str) and len(a) == 1 and len(b) == 1 and a in letters and b in letters):
                raise ValueError(f"complement maps {a!r} to {b!r}: both must be letters of the alphabet")
            to[letters.index(a)] = letters.index(b)
        # a residue t of the other strand stands opposite to[t] of this one: scores'[i, t] = scores[Q - 1 - i, to[t]]
        scores = self.scores[::-1][:, to]
        lookup = np.arange(256, dtype=np.uint8)
        lookup[:len(to)] = to
        return Pssm(scores, self.alphabet, lookup[self.consensus[::-1]])

    @classmethod
    def from_columns(cls, columns: "ProfileColumns", prior: "Pssm", background, lam: float, *,
                     pseudocount: float = 10.0) -> "Pssm":
        """The PSSM of the next round from the columns of this round's hits. ``prior``: a `Pssm` of the same length and
        alphabet - the round's query, ``Pssm.from_sequence(...)`` in round 1; ``background``: one frequency ``p_a`` per
        letter; ``lam``: the scale of the scores (`matrix_lambda`). In float64, with ``f = columns.frequencies()``,
        ``alpha_i = max(k_i - 1, 0)`` (``k_i = columns.distinct``), ``beta = pseudocount``, ``g_ia = p_a exp(lam
        prior[i][a])`` normalised over the letters with ``p_a > 0`` and ``q_ia = (alpha_i f_ia + beta g_ia) / (alpha_i +
        beta)``: the new score is ``rint(ln(q_ia / p_a) / lam)``, clipped to int16. A letter with ``p_a == 0`` keeps the
        prior's score, a position whose weighted row is empty the prior's row; the consensus is the prior's. A position
        only the query covers has ``alpha = 0``: it keeps its prior row up to the normalisation."""
        if not isinstance(columns, ProfileColumns):
            raise TypeError(f"Argument 'columns' has incorrect type (expected ProfileColumns, got {type(columns).__name__})")
        if not isinstance(prior, Pssm):
            raise TypeError(f"Argument 'prior' has incorrect type (expected Pssm, got {type(prior).__name__})")
        if prior.alphabet != columns.alphabet or len(prior) != len(columns):
            raise ValueError("columns and prior differ in length or alphabet")
        A = len(prior.alphabet)
        p = np.asarray(background, dtype=np.float64)
        if p.shape != (A,) or not np.all(np.isfinite(p)) or np.any(p < 0) or not np.any(p > 0):
            raise ValueError(f"background must hold {A} frequencies, none negative, one positive at least")
        lam, beta = float(lam), float(pseudocount)
        if not (np.isfinite(lam) and lam > 0):
            raise ValueError("lam must be finite and positive")
        if not (np.isfinite(beta) and beta > 0):
            raise ValueError("pseudocount must be finite and positive")
        letters = p > 0
        f = columns.frequencies()
        alpha = np.maximum(columns.distinct.astype(np.float64) - 1.0, 0.0)[:, None]
        g = np.zeros((len(prior), A), dtype=np.float64)
        g[:, letters] = p[letters] * np.exp(lam * prior.scores[:, letters].astype(np.float64))
        g /= g.sum(axis=1, keepdims=True) if len(prior) else 1.0
        q = (alpha * f + beta * g) / (alpha + beta)
        scores = np.array(prior.scores, dtype=np.int64)
        fresh = np.rint(np.log(q[:, letters] / p[letters]) / lam)
        scores[:, letters] = np.clip(fresh, -(2 ** 15), 2 ** 15 - 1).astype(np.int64)
        empty = columns.weighted[:, :A].sum(axis=1) == 0
        scores[empty] = prior.scores[empty]
        return cls(scores, prior.alphabet, prior.consensus)

    @property
    def consensus_sequence(self) -> str:
        """The consensus as text; ``-`` where a position has no residue."""
        letters = np.frombuffer((self.alphabet.letters + "-" * (256 - len(self.alphabet))).encode("ascii"), dtype=np.uint8)
        return letters[self.consensus].tobytes().decode("ascii")

    def __len__(self) -> int:
        return len(self.scores)

    def __eq__(self, other):
        if not isinstance(other, Pssm):
            return NotImplemented
        return (self.alphabet == other.alphabet and np.array_equal(self.scores, other.scores) and
                np.array_equal(self.consensus, other.consensus))

    __hash__ = None

    def __reduce__(self):
        return type(self), (np.array(self.scores), self.alphabet.letters, np.array(self.consensus))

    def __repr__(self):
        return f"{type(self).__name__}(<{len(self)} x {len(self.alphabet)}>, consensus={self.consensus_sequence!r})"


class ProfileColumns:
    """What `Aligner.profile_columns` returns: the query-anchored columns of a query and its aligned targets
    (include/miopal.h, miopalProfileColumns). With ``Q`` positions, ``A`` letters and ``n`` targets: ``counts`` and
    ``weighted`` are int64 of shape ``(Q, A + 1)`` - per position the members that show letter ``a`` there, and the
    sum of their weights; column ``A`` is the gap letter (a query position against a gap). ``member_weights``: int64,
    ``n + 1`` Henikoff position-based weights in 32.32 fixed point (``WEIGHT_ONE`` is 1.0), the query first. ``msa``:
    uint8 ``(n + 1, Q)`` - a letter, ``A`` for the gap, 255 where the member's alignment does not cover the position -
    or None when it was not asked for. ``alphabet``; ``consensus``: the query's codes (255: no residue)."""

    WEIGHT_ONE = _capi.MIOPAL_PROFILE_WEIGHT_ONE
    UNCOVERED = _capi.PROFILE_UNCOVERED
    __slots__ = ("counts", "weighted", "member_weights", "alphabet", "consensus", "msa")

    def __init__(self, counts, weighted, member_weights, alphabet, consensus, msa=None):
        if isinstance(alphabet, str):
            alphabet = Alphabet(alphabet)
        elif not isinstance(alphabet, Alphabet):
            raise TypeError(f"expected str or Alphabet, found {type(alphabet).__name__}")
        self.alphabet = alphabet
        self.consensus = np.array(consensus, dtype=np.uint8).ravel()
        shape = (len(self.consensus), len(alphabet) + 1)
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.weighted = np.ascontiguousarray(weighted, dtype=np.int64)
        if self.counts.shape != shape or self.weighted.shape != shape:
            raise ValueError(f"counts and weighted must have shape {shape}")
        self.member_weights = np.ascontiguousarray(member_weights, dtype=np.int64).ravel()
        self.msa = None if msa is None else np.ascontiguousarray(msa, dtype=np.uint8)
        if self.msa is not None and self.msa.shape != (len(self.member_weights), shape[0]):
            raise ValueError("msa must hold one row per member and one entry per position")

    @classmethod
    def of_query(cls, codes, alphabet, return_msa: bool = False) -> "ProfileColumns":
        """The profile of the query alone (no targets), in integers on the host: every position with a residue shows
        one letter once, and the query's weight is one per such position."""
        codes = np.array(codes, dtype=np.uint8).ravel()
        A = len(alphabet)
        at = np.flatnonzero(codes < A)
        weight = len(at) * cls.WEIGHT_ONE
        counts = np.zeros((len(codes), A + 1), dtype=np.int64)
        weighted = np.zeros((len(codes), A + 1), dtype=np.int64)
        counts[at, codes[at]] = 1
        weighted[at, codes[at]] = weight
        msa = np.where(codes < A, codes, cls.UNCOVERED).astype(np.uint8)[None, :] if return_msa else None
        return cls(counts, weighted, [weight], alphabet, codes, msa)

    @property
    def distinct(self) -> np.ndarray:
        """``k_i``: the letters (the gap is none) that occur at position ``i``."""
        return np.count_nonzero(self.counts[:, :len(self.alphabet)], axis=1).astype(np.int64)

    def frequencies(self) -> np.ndarray:
        """``weighted[:, :A]`` normalised per position, float64; a position with nothing in it gives zeros."""
        w = self.weighted[:, :len(self.alphabet)].astype(np.float64)
        total = w.sum(axis=1, keepdims=True)
        return np.divide(w, total, out=np.zeros_like(w), where=total > 0)

    def __len__(self) -> int:
        return len(self.consensus)

    def __repr__(self):
        return f"{type(self).__name__}(<{len(self)} x {len(self.alphabet) + 1}>, members={len(self.member_weights)})"


def matrix_lambda(scoring_matrix, background) -> float:
    """The scale of a scoring matrix under a background: the positive root ``lam`` of ``sum_ab p_a p_b exp(lam S_ab) =
    1``, by bisection. ``scoring_matrix``: a `ScoringMatrix` or a name; ``background``: one frequency per letter
    (normalised here). ValueError when the expected score is not negative or no entry between letters of positive
    frequency is positive - there is no such root then."""
    matrix = resolve_scoring_matrix(scoring_matrix, "found")
    n = len(matrix.alphabet)
    S = np.asarray(matrix.matrix, dtype=np.float64).reshape(n, n)
    p = np.asarray(background, dtype=np.float64)
    if p.shape != (n,) or not np.all(np.isfinite(p)) or np.any(p < 0) or not np.any(p > 0):
        raise ValueError(f"background must hold {n} frequencies, none negative, one positive at least")
    p = p / p.sum()
    pp = np.outer(p, p)
    held = pp > 0
    if not np.sum(pp[held] * S[held]) < 0:
        raise ValueError("the expected score under the background is not negative")
    if not np.any(S[held] > 0):
        raise ValueError("no positive score between letters of the background")

    def excess(lam):
        return float(np.sum(pp[held] * np.exp(lam * S[held]))) - 1.0
    lo, hi = 0.0, 1.0
    while excess(hi) <= 0:   # (convex, 0 at 0 with a negative slope, unbounded: positive from the root on)
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if excess(mid) <= 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


class BatchResultArrays:
    """Results of a batched search as 2-D arrays (`Aligner.align_many_arrays`): ``score`` and, for
    ``mode="end"``, ``query_end`` / ``target_end``, ``int32`` of shape ``(queries, targets)``.
    ``arrays[i]`` is the `ResultArrays` of query ``i``."""

    def __init__(self, mode: str, start: int, query_lengths, out):
        self.mode = mode
        self.start = start
        self.query_lengths = list(query_lengths)
        self.score = out["score"]
        self.query_end = out.get("end_q")
        self.target_end = out.get("end_t")

    def __len__(self) -> int:
        return self.score.shape[0]

    def __getitem__(self, i: int) -> "ResultArrays":
        m = len(self)
        if i < 0:
            i += m
        if i < 0 or i >= m:
            raise IndexError(i)
        out = {"score": self.score[i]}
        if self.mode == "end":
            out.update(end_q=self.query_end[i], end_t=self.target_end[i])
        return ResultArrays(self.mode, self.start, self.query_lengths[i], None, out)

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class ResultArrays:
    """Results of one search as arrays (`Aligner.align_arrays`).

    Attributes (``int32`` arrays, one entry per target of the slice): ``score``; for the
    ``end`` and ``full`` modes ``query_end``, ``target_end``; for ``full`` also
    ``query_start``, ``target_start``, ``target_length`` and the alignments as one ``uint8``
    buffer ``operations`` (codes of ``src/pyopal/opal.pxd:21-24``) with ``operation_offsets``
    (``int64``, n + 1 entries). Indexing and iteration yield `ScoreResult` / `EndResult` /
    `FullResult` objects equal to those of `Aligner.align`.
    """

    def __init__(self, mode: str, start: int, query_length: int, target_lengths, out):
        self.mode = mode
        self.start = start
        self.query_length = query_length
        self.score = out["score"]
        self.query_end = out.get("end_q")
        self.target_end = out.get("end_t")
        self.query_start = out.get("start_q")
        self.target_start = out.get("start_t")
        self.operations = out.get("aln_flat")
        self.operation_offsets = out.get("aln_off")
        self.target_length = target_lengths if mode == "full" else None

    def __len__(self) -> int:
        return len(self.score)

    def alignment(self, k: int) -> str:
        """The operations of target ``k`` of the slice over ``MDIX`` (`FullResult.alignment`)."""
        if self.mode != "full":
            raise ValueError("alignments are only computed in 'full' mode")
        lo, hi = self.operation_offsets[k], self.operation_offsets[k + 1]
        return self.operations[lo:hi].tobytes().translate(_OPS_TO_TEXT).decode("ascii")

    def __getitem__(self, k: int):
        n = len(self)
        if k < 0:
            k += n
        if k < 0 or k >= n:
            raise IndexError(k)
        index = self.start + k
        if self.mode == "score":
            return ScoreResult(index, int(self.score[k]))
        if self.mode == "end":
            return EndResult(index, int(self.score[k]), int(self.query_end[k]), int(self.target_end[k]))
        return FullResult(index, int(self.score[k]), int(self.query_end[k]), int(self.target_end[k]),
                          int(self.query_start[k]), int(self.target_start[k]), self.query_length,
                          int(self.target_length[k]), self.alignment(k))

    def __iter__(self):
        return (self[k] for k in range(len(self)))


_OPS_TO_TEXT = bytes.maketrans(bytes([0, 1, 2, 3]), b"MDIX")  # src/pyopal/lib.pyx:991


def _int_matrix_array(matrix) -> np.ndarray:
    if isinstance(matrix, array.array):
        return np.frombuffer(matrix, dtype=np.int32)
    return np.ascontiguousarray(matrix, dtype=np.int32)
