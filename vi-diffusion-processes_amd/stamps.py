"""One staleness key for every cached device result: a `Stamp` records what the result was computed from, `wrote` tells torch about a
write it did not see (a library call on raw pointers, a graph replay), so that the stamps on the written tensors stop matching."""
import weakref

import torch


class Stamp:
    """Stamp(*parts): a tensor part is recorded as a weak reference plus its version, any other part by value.  `matches(*parts)` is
    true only for the same number of parts, every tensor part the SAME OBJECT at the same version and every value part equal.  A tensor
    that has died never matches: no address is compared (the allocator reuses them) and no key keeps a tensor alive."""
    __slots__ = ("_parts",)

    def __init__(self, *parts):
        self._parts = [(weakref.ref(p), p._version) if isinstance(p, torch.Tensor) else (None, p) for p in parts]

    def matches(self, *parts):
        if len(parts) != len(self._parts):
            return False
        for (ref, val), p in zip(self._parts, parts):
            if ref is None:
                if isinstance(p, torch.Tensor) or val != p:
                    return False
            elif p is None or ref() is not p or val != p._version:      # (a dead reference gives None: never a match)
                return False
        return True


def wrote(*tensors):
    """The tensors (None entries skipped) were written behind torch's back: bump their versions."""
    for t in tensors:
        if t is not None:
            torch.autograd.graph.increment_version(t)
