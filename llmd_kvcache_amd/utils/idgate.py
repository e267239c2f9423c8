"""Readers-writer gate around a dense id space.

Pod ids are handed out by the registry and travel through two kinds of
span: a writer turns a name into an id and launches with it later; a
reader stages id-indexed arguments and later labels an id-ordered result
with names.  A renumbering of the ids must not fall inside either.  Both
kinds take the SHARED side for the whole span; the renumbering takes the
EXCLUSIVE side.

 - The shared side is re-entrant per thread: only a thread's outermost
   entry can wait, a nested one never does - not even while an exclusive
   entrant is waiting, which is what keeps nested spans free of deadlock.
 - A waiting exclusive entrant holds back NEW outermost shared entrants,
   so a steady stream of readers cannot starve it.
 - The holder of the exclusive side may enter either side again.
 - Asking for the exclusive side from inside a shared span can never be
   granted and raises.
"""

from __future__ import annotations

import threading


class _Side:
    __slots__ = ("_enter", "_exit")

    def __init__(self, enter, exit_):
        self._enter = enter
        self._exit = exit_

    def __enter__(self):
        self._enter()
        return self

    def __exit__(self, *exc):
        self._exit()
        return False


class IdGate:
    def __init__(self):
        self._cond = threading.Condition(threading.Lock())
        self._readers = 0          # threads inside an outermost shared span
        self._writer = None        # ident of the exclusive holder
        self._writer_depth = 0
        self._waiting_writers = 0
        self._local = threading.local()
        self.shared = _Side(self._enter_shared, self._exit_shared)
        self.exclusive = _Side(self._enter_exclusive, self._exit_exclusive)

    # -- shared --------------------------------------------------------
    def _enter_shared(self) -> None:
        loc = self._local
        depth = getattr(loc, "depth", 0)
        if depth == 0 and self._writer != threading.get_ident():
            with self._cond:
                while self._writer is not None or self._waiting_writers:
                    self._cond.wait()
                self._readers += 1
            loc.counted = True
        elif depth == 0:
            loc.counted = False    # inside this thread's exclusive span
        loc.depth = depth + 1

    def _exit_shared(self) -> None:
        loc = self._local
        loc.depth -= 1
        if loc.depth == 0 and loc.counted:
            with self._cond:
                self._readers -= 1
                if self._readers == 0:
                    self._cond.notify_all()

    # -- exclusive -----------------------------------------------------
    def _enter_exclusive(self) -> None:
        me = threading.get_ident()
        if self._writer == me:
            self._writer_depth += 1
            return
        if getattr(self._local, "depth", 0):
            raise RuntimeError(
                "exclusive id gate requested inside a shared span")
        with self._cond:
            self._waiting_writers += 1
            try:
                while self._writer is not None or self._readers:
                    self._cond.wait()
            finally:
                self._waiting_writers -= 1
            self._writer = me
            self._writer_depth = 1

    def _exit_exclusive(self) -> None:
        self._writer_depth -= 1
        if self._writer_depth == 0:
            with self._cond:
                self._writer = None
                self._cond.notify_all()

    # -- introspection (tests) -----------------------------------------
    @property
    def waiting_exclusive(self) -> int:
        with self._cond:
            return self._waiting_writers
