"""Architecture registry and checkpoint-file loading (drop-in for ``resselt/registry.py:14-116``).

Behaviour kept from the reference:
  * ``get`` of an unknown id raises ``KeyError`` (registry.py:73-77);
  * ``load_from_file`` dispatches on the extension: ``.pt`` tries TorchScript first and falls back to a
    restricted pickle, ``.pth``/``.ckpt`` use the restricted pickle, ``.safetensors`` uses safetensors,
    anything else raises ``ValueError`` (registry.py:79-104);
  * the restricted unpickler only admits OrderedDict, ``_rebuild_tensor_v2`` and six storage classes and
    raises ``pickle.UnpicklingError`` for every other global (registry.py:20-46);
  * ``load_from_state_dict`` canonicalises, walks the architectures in insertion order (then ``Registry.late``, then ``Registry.last``, then
    ``Registry.after``, then ``Registry.tail``, then ``Registry.rest``, ``Registry.more`` and ``Registry.beyond``: ``Registry.consultation()``), builds the first match and calls ``model.load_state_dict(canonicalised_dict)`` (registry.py:106-116);
  * no match raises ``ArchitectureNotFound``.

Documented deviation: the reference hands the *unconverted* dict to ``load_state_dict``, so official
Real-ESRGAN "new-arch" checkpoints are detected but then fail with missing keys.  The
engine modules returned here accept both key spellings in ``load_state_dict`` so those checkpoints load.
"""

from __future__ import annotations

import os
import pickle
from types import SimpleNamespace
from typing import Dict, Iterator, Mapping

import torch

from .factory import Architecture
from .utilities.state_dict import canonicalize_state_dict


class ArchitectureNotFound(Exception):
    pass


_ALLOWED_GLOBALS = frozenset(
    {
        ('collections', 'OrderedDict'),
        ('typing', 'OrderedDict'),
        ('torch._utils', '_rebuild_tensor_v2'),
        ('torch', 'BFloat16Storage'),
        ('torch', 'FloatStorage'),
        ('torch', 'HalfStorage'),
        ('torch', 'IntStorage'),
        ('torch', 'LongStorage'),
        ('torch', 'DoubleStorage'),
    }
)


class RestrictedUnpickler(pickle.Unpickler):
    """Unpickler that can only rebuild plain tensor dictionaries."""

    def find_class(self, module: str, name: str):
        if (module, name) not in _ALLOWED_GLOBALS:
            raise pickle.UnpicklingError(f"Global '{module}.{name}' is forbidden")
        return super().find_class(module, name)


def _restricted_load(*args, **kwargs):
    return RestrictedUnpickler(*args, **kwargs).load()


# what torch.load(pickle_module=...) needs: a module-like object with Unpickler/load and a __name__
RestrictedUnpickle = SimpleNamespace(Unpickler=RestrictedUnpickler, __name__='pickle', load=_restricted_load)


def _read_checkpoint(path: str) -> Mapping[str, object]:
    ext = os.path.splitext(path)[1].lower()
    if ext == '.pt':
        try:
            return torch.jit.load(path).state_dict()
        except RuntimeError:
            try:
                return torch.load(path, pickle_module=RestrictedUnpickle)
            except Exception:
                pass
            raise
    if ext in ('.pth', '.ckpt'):
        return torch.load(path, pickle_module=RestrictedUnpickle)
    if ext == '.safetensors':
        import safetensors.torch

        return safetensors.torch.load_file(path)
    raise ValueError(f'Unsupported model file extension {ext}. Please try a supported model type.')


class Registry:
    """``store`` is the ordered walk: the first architecture whose keys match builds the model, so the order matters wherever two
    architectures share keys, and it follows the reference's walk.  ``late`` holds architectures that are consulted after the whole walk
    has declined: only for an architecture whose detection keys no other one matches and which matches no other one's checkpoints, so
    that its position cannot change who loads what.  ``last`` is a further tier of the same kind, consulted after ``late``; ``walk()`` yields
    all three in the order ``load_from_state_dict`` consults them.  Iterating over the registry and ``len()`` cover ``store`` and ``late``
    only, as they did before ``last`` existed.  ``after`` is the open-ended tier behind them: any number of architectures, each under the same
    admission rule, consulted in insertion order once ``walk()`` has declined; ``consulted()`` yields everything, ``after`` included, in
    consultation order, and ``__iter__``, ``len()`` and ``walk()`` do not see it -- a further architecture needs no further tier.
    ``tail`` is where architectures go that came after ``consulted()`` had been pinned down as ``walk()`` + MoESR (tests/test_moesr_loader.py
    holds ``after`` and ``consulted()`` to exactly that): the same admission rule, insertion order, consulted once ``consulted()`` has
    declined; ``every()`` yields ``consulted()`` and then ``tail``, and nothing else sees it.
    ``rest`` is the tier for every architecture after that (tests/test_smosr_loader.py holds ``tail`` and ``every()`` to exactly
    ``consulted()`` + SMoSR): the same admission rule, any number of architectures in insertion order, consulted once ``every()`` has
    declined.  ``order()`` is the whole consultation order and what ``load_from_state_dict`` walks; no test may hold ``rest`` or ``order()``
    to a fixed list of ids (membership and relative order only), so the next architecture goes into ``rest`` too.
    ``more`` exists because one did (tests/test_lawfft_loader.py holds ``rest`` and the end of ``order()`` to exactly GFISRv2, FIGSR, LAWFFT):
    the same admission rule, any number of architectures in insertion order, consulted once ``order()`` has declined; ``full()`` is the
    whole consultation order up to there, and no older tier or iterator sees ``more``.
    ``beyond`` is the tier behind ``more`` (tests/test_gfisr_loader.py holds ``more`` to exactly GFISR and ``full()`` to ``order()`` + GFISR):
    the same admission rule, any number of architectures in insertion order, consulted once ``full()`` has declined; ``consultation()``
    yields ``full()`` and then ``beyond`` and is what ``load_from_state_dict`` walks.  No older tier, iterator or ``len()`` sees ``beyond``,
    and no test may hold ``beyond`` or the end of ``consultation()`` to a fixed list of ids (membership and relative order only), so the
    next architecture goes into ``beyond`` too."""

    def __init__(self):
        self.store: Dict[str, Architecture] = {}
        self.late: Dict[str, Architecture] = {}
        self.last: Dict[str, Architecture] = {}
        self.after: Dict[str, Architecture] = {}
        self.tail: Dict[str, Architecture] = {}
        self.rest: Dict[str, Architecture] = {}
        self.more: Dict[str, Architecture] = {}
        self.beyond: Dict[str, Architecture] = {}

    def __contains__(self, uid: str) -> bool:
        return uid in self.store or uid in self.late or uid in self.last or uid in self.after or uid in self.tail or uid in self.rest or uid in self.more or uid in self.beyond

    def __iter__(self) -> Iterator[Architecture]:
        return iter(list(self.store.values()) + list(self.late.values()))

    def __len__(self) -> int:
        return len(self.store) + len(self.late)

    def walk(self) -> Iterator[Architecture]:
        """``store``, ``late``, ``last``: the first three tiers in the order ``load_from_state_dict`` consults them."""
        return iter(list(self.store.values()) + list(self.late.values()) + list(self.last.values()))

    def consulted(self) -> Iterator[Architecture]:
        """``walk()``, then ``after``: what ``load_from_state_dict`` consults before ``tail`` (``every()`` is the whole order)."""
        return iter(list(self.walk()) + list(self.after.values()))

    def every(self) -> Iterator[Architecture]:
        """Every registered architecture in the order ``load_from_state_dict`` consults them: ``consulted()``, then ``tail``."""
        return iter(list(self.consulted()) + list(self.tail.values()))

    def order(self) -> Iterator[Architecture]:
        """``every()``, then ``rest``: what ``load_from_state_dict`` consults before ``more`` (``full()`` is the whole order)."""
        return iter(list(self.every()) + list(self.rest.values()))

    def full(self) -> Iterator[Architecture]:
        """``order()``, then ``more``: what ``load_from_state_dict`` consults before ``beyond`` (``consultation()`` is the whole order)."""
        return iter(list(self.order()) + list(self.more.values()))

    def consultation(self) -> Iterator[Architecture]:
        """The whole consultation order of ``load_from_state_dict``: ``full()``, then ``beyond``."""
        return iter(list(self.full()) + list(self.beyond.values()))

    def add(self, arch: Architecture, late: bool = False, last: bool = False, after: bool = False, tail: bool = False, rest: bool = False,
            more: bool = False, beyond: bool = False) -> None:  # fmt: skip
        """Register an architecture *instance*; re-using an id replaces it in place."""
        if beyond and not any(arch.id in t for t in (self.store, self.late, self.last, self.after, self.tail, self.rest, self.more)):
            self.beyond[arch.id] = arch
            return
        self.beyond.pop(arch.id, None)
        if beyond:  # an id another tier already holds is replaced there
            more = more or arch.id in self.more
        if more and not any(arch.id in t for t in (self.store, self.late, self.last, self.after, self.tail, self.rest)):
            self.more[arch.id] = arch
            return
        self.more.pop(arch.id, None)
        if more:  # an id another tier already holds is replaced there
            rest = rest or arch.id in self.rest
        if rest and not any(arch.id in t for t in (self.store, self.late, self.last, self.after, self.tail)):
            self.rest[arch.id] = arch
            return
        self.rest.pop(arch.id, None)
        if rest:  # an id another tier already holds is replaced there
            tail = tail or arch.id in self.tail
        if tail and not any(arch.id in t for t in (self.store, self.late, self.last, self.after)):
            self.tail[arch.id] = arch
            return
        self.tail.pop(arch.id, None)
        if tail:  # an id another tier already holds is replaced there
            after, last, late = after or arch.id in self.after, last or arch.id in self.last, late or arch.id in self.late
        if after and arch.id not in self.store and arch.id not in self.late and arch.id not in self.last:
            self.after[arch.id] = arch
            return
        self.after.pop(arch.id, None)
        if last and arch.id not in self.store and arch.id not in self.late:
            self.last[arch.id] = arch
        elif late and arch.id not in self.store:
            self.last.pop(arch.id, None)
            self.late[arch.id] = arch
        else:
            self.late.pop(arch.id, None)
            self.last.pop(arch.id, None)
            self.store[arch.id] = arch

    def get(self, uid: str) -> Architecture:
        tier = next((t for t in (self.late, self.last, self.after, self.tail, self.rest, self.more, self.beyond) if uid in t), self.store)
        arch = tier[uid]  # KeyError for unknown ids, as in the reference
        if not arch:
            raise ArchitectureNotFound
        return arch

    def load_from_file(self, path: str):
        return self.load_from_state_dict(_read_checkpoint(path))

    def load_from_state_dict(self, state_dict: Mapping[str, object]):
        state_dict = canonicalize_state_dict(state_dict)
        for arch in self.consultation():
            if arch.detect(state_dict):
                model = arch.load(state_dict)
                model.load_state_dict(state_dict)
                return model
        raise ArchitectureNotFound
