"""Deferred parameter-gradient finishing (csrc/pgrad.hip, include/e2ep.h e2ep_defer_*).

The split-slab sum of a conv weight gradient, the LayerNorm dgamma / dbeta partial sum and the
squeeze-excitation weight gradient feed nothing in the backward.  Inside a ParamGradDefer
scope the library records those launches instead of issuing them, and the scope's exit runs
them batched, one launch per kind, on the current stream: same sums, same order, same bits.

The scope spans the forward and the backward.  In the forward every op notes the parameters
it uses (note); in the backward an op defers only when each of its parameters is a leaf that
the forward used exactly once and whose .grad is still unset (call): a second gradient of a
parameter is added into .grad in place by autograd, and the gradient of a non-leaf is read by
the next backward node, and either would read the first result before the flush has written
it.  Everything else launches immediately, as without a scope.

The scope keeps alive what the pending records read (slab workspaces, SE tensors) until the
flush has been launched; otherwise the caching allocator could hand that memory out again
first (inside a graph capture, the reference is what keeps the private pool from reusing the
block).  It never holds a reference to an output gradient: autograd takes a gradient tensor
over as .grad only while nothing else refers to it, and clones it — unwritten — otherwise.

The stack and the scope are module-level, not thread-local: autograd runs the backward nodes
on its own thread while the scope is entered and left on the caller's."""
from . import _lib

_SCOPES = []  # active scopes (at most one: the library takes one at a time)


class ParamGradDefer:
    """with ParamGradDefer(): forward; backward  — the flush happens at a clean exit, on the
    stream current there, which must be ordered after the backward (autograd joins the
    streams its nodes ran on before backward() returns; conv._Fork joins its side stream).
    uses: the use counts of an earlier scope over the same forward (a backward continued in a
    second scope: the segmented train step's stage 2)."""

    def __init__(self, uses=None):
        self.uses = {} if uses is None else uses  # id(parameter) -> [parameter, uses in the forward]
        self.keep = []                            # tensors the pending records read

    def __enter__(self):
        _lib.call("e2ep_defer_begin")
        _SCOPES.append(self)
        return self

    def __exit__(self, *exc):
        _SCOPES.pop()
        try:
            # nothing recorded (key 37 = 1, or a step on host tensors, where there is no
            # stream to name): the scope just closes
            if exc[0] is None and _lib.call_raw("e2ep_defer_pending"):
                _lib.call("e2ep_defer_flush", _lib.stream())
            else:
                _lib.call("e2ep_defer_abort")
        finally:
            self.keep = []
        return False

    def ok(self, keys):
        if keys is None:
            return False
        for k in keys:
            ent = self.uses.get(k)
            if ent is None or ent[1] != 1 or not ent[0].is_leaf or ent[0].grad is not None:
                return False
        return True


def active():
    return _SCOPES[-1] if _SCOPES else None


def note(*params):
    """Forward: count one use of each parameter (None entries skipped); returns the keys the
    backward passes to call(), or None outside a scope."""
    if not _SCOPES:
        return None
    uses = _SCOPES[-1].uses
    keys = []
    for p in params:
        if p is None:
            continue
        ent = uses.get(id(p))
        if ent is None:
            uses[id(p)] = [p, 1]
        else:
            ent[1] += 1
        keys.append(id(p))
    return tuple(keys)


ANY = object()


class call:
    """with defer.call(keys) as dc: dc.keep(ws, ...); _lib.call(<a deferring entry point>)

    Around one library call that may record a deferred launch.  With `keys` (note()'s result
    for the op's parameters) the call is held to the immediate path unless the scope allows
    every one of them; without, it defers whenever a scope is open (direct calls, whose caller
    answers for the outputs).  The tensors given to keep() stay referenced by the scope until
    the flush if, and only if, the call left a record."""

    def __init__(self, keys=ANY):
        self.scope = _SCOPES[-1] if _SCOPES else None
        self.keys = keys
        self.tensors = ()
        self.held = False

    def keep(self, *tensors):
        self.tensors = tensors

    def __enter__(self):
        if self.scope is not None:
            if self.keys is not ANY and not self.scope.ok(self.keys):
                self.held = True
                _lib.call_raw("e2ep_defer_hold", 1)
            else:
                self.before = _lib.call_raw("e2ep_defer_pending")
        return self

    def __exit__(self, *exc):
        if self.scope is None:
            return False
        if self.held:
            _lib.call_raw("e2ep_defer_hold", 0)
        elif _lib.call_raw("e2ep_defer_pending") > self.before:
            self.scope.keep.extend(t for t in self.tensors if t is not None)
        return False
