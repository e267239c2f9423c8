"""Python wrapper for the native (C++) wire front.

The wirefront (ops/csrc/wirefront.cpp) owns the sockets: epoll io
threads parse HTTP/1.1 + JSON natively and a batcher thread crosses
into Python exactly once per micro-batch through the two callbacks
below.  Python's role per batch is the already-hot scoring path:
parallel C++ chain (hash_chain_batch) + one fused probe/score kernel,
or the chain on the GPU as well where the indexer's read route says so.

    svc = WireIndexerService(indexer)
    port = svc.start(port=8080, n_io=4)
    ...
    svc.stop()

Endpoints (JSON over HTTP/1.1 keep-alive, pipelining supported):
    POST /score   {"model": m, "tokens": [...]}  pre-tokenized fast path
                  {"model": m, "prompt": "..."}  text (tokenization incl.)
                  optional {"pods": ["p1", ...]} candidate filter
    GET  /health

The reference's shipped service is the Go HTTP binary
(examples/kv_events/online/main.go:269-365); this is its MI355X-native
equivalent with the request path in C++ instead of Go.
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

from ..indexer import Indexer, pack_token_lists, plan_read_route
from ..utils import hashing


class WireIndexerService:
    def __init__(self, indexer: Indexer, max_batch: int = 4096,
                 n_batchers: int = 2):
        from ..ops import cpu_ext

        ops = cpu_ext.require()
        if not hasattr(ops, "WireFront"):
            raise RuntimeError(
                "native extension built without the wirefront - rebuild")
        algo = indexer.tokens_processor.config.hash_algo
        if algo not in hashing.NATIVE_ALGO_IDS:
            raise ValueError(
                f"wirefront requires a chain hash with a native "
                f"implementation ({sorted(hashing.NATIVE_ALGO_IDS)}); "
                f"got {algo!r}")
        self._algo_id = hashing.NATIVE_ALGO_IDS[algo]
        self.indexer = indexer
        self._front = ops.WireFront(self._score_tokens_cb,
                                    self._score_text_cb, max_batch,
                                    n_batchers)
        self._running = False

    # -- lifecycle -----------------------------------------------------
    def start(self, host: str = "", port: int = 0, n_io: int = 2) -> int:
        """Binds and serves; returns the bound port (port=0 -> ephemeral).
        host="" binds loopback; use "0.0.0.0" to expose."""
        bound = self._front.start(host, port, n_io)
        self._running = True
        return bound

    def stop(self) -> None:
        if self._running:
            self._running = False
            self._front.stop()

    @property
    def port(self) -> int:
        return self._front.port()

    def stats(self) -> Tuple[int, int]:
        """(requests served, micro-batches dispatched)."""
        return self._front.requests(), self._front.batches()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.stop()
        return False

    # -- batch callbacks (invoked by the C++ batcher) ------------------
    # The Python part of a batch is only id/filter/weight staging (~us);
    # the heavy work runs inside ops.wire_score_flat, which RELEASES the
    # GIL - so multiple C++ batcher threads overlap and io threads are
    # never stalled behind scoring.
    def _stage(self, model: str, pods: Sequence[str]):
        idx = self.indexer.kv_block_index()
        tp = self.indexer.tokens_processor
        a = idx.score_args(model, pods, self.indexer.config.backend_configs)
        from ..kvblock.gpu_index import _to_i64

        return (idx, a.model_id, a.filter_words, a.weights, a.num_pods,
                a.n_tiers, _to_i64(tp.config.init_hash()), tp.block_size)

    def _device_chain(self, idx, offsets, bs) -> int:
        """The per-batch routing decision (indexer.plan_read_route) as
        wire_score_flat's trailing argument."""
        tp = self.indexer.tokens_processor
        route = plan_read_route(offsets, bs, tp.config.hash_algo,
                                idx.table.is_cuda, self.indexer.config)
        return 1 if route.device else 0

    @staticmethod
    def _run_flat(idx, *args):
        if idx.table.is_cuda:
            return idx.table.ops.wire_score_flat(*args)
        # CPU tables are single-writer/locked-reader (gpu_index.py
        # fused_scores takes the same lock); the op releases the GIL so
        # the lock is what serializes against concurrent event applies
        with idx._write_lock:
            return idx.table.ops.wire_score_flat(*args)

    def _score_tokens_cb(self, model: str, pods: Sequence[str],
                         tokens_flat, offsets):
        # pod ids stand still from staging to naming: wire_score_flat
        # returns host scores, so nothing id-ordered outlives the span
        with self.indexer.kv_block_index().registry.ids_shared():
            (idx, model_id, filt, weights, num_pods, n_tiers, init,
             bs) = self._stage(model, pods)
            scores = self._run_flat(
                idx, *idx.table._t(), tokens_flat, offsets, model_id, filt,
                weights, num_pods, idx.table.next_epoch(), init, bs, n_tiers,
                self._algo_id, self._device_chain(idx, offsets, bs))
            return scores, list(idx.registry.id_to_pod)

    def _score_text_cb(self, model: str, pods: Sequence[str],
                       prompts: List[str]):
        import torch

        pool = self.indexer.tokenizers_pool
        if hasattr(pool, "tokenize_batch"):
            token_lists = pool.tokenize_batch(list(prompts), model)
        else:  # custom pool injected without the batch API
            token_lists = [pool.tokenize(None, p, model) for p in prompts]
        flat_t, off_t = pack_token_lists(token_lists)
        with self.indexer.kv_block_index().registry.ids_shared():
            (idx, model_id, filt, weights, num_pods, n_tiers, init,
             bs) = self._stage(model, pods)
            scores = self._run_flat(
                idx, *idx.table._t(), flat_t, off_t, model_id, filt, weights,
                num_pods, idx.table.next_epoch(), init, bs, n_tiers,
                self._algo_id, self._device_chain(idx, off_t, bs))
            names = list(idx.registry.id_to_pod)
        # 4-tuple: the C++ side feeds elements 2/3 (int32 tokens +
        # offsets) into its prompt cache so repeats skip Python
        return (scores, names, flat_t.to(torch.int32), off_t)
