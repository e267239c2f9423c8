// bindings.cpp - pybind11 module _kvidx_C: CPU ops always, HIP ops when
// built with KVIDX_WITH_HIP (the default on this ROCm image; hipcc
// cross-compiles gfx950 without a GPU present).

#include "kvidx_ops.h"

namespace kvidx::wire {
void register_wirefront(pybind11::module_& m);  // wirefront.cpp
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native KV-block index ops (CPU reference + gfx950 HIP)";
  // Chain ops take a trailing native algo id (utils/hashing.py
  // NATIVE_ALGO_IDS); 0 = fnv-64a is the default everywhere.
  m.def("tokens_to_chunk_hashes", &kvidx::tokens_to_chunk_hashes,
        py::arg("tokens"), py::arg("parent"), py::arg("block_size"),
        py::arg("algo") = 0);
  m.def("hash_chain_batch", &kvidx::hash_chain_batch,
        py::arg("tokens"), py::arg("offsets"), py::arg("parents"),
        py::arg("block_size"), py::arg("algo") = 0);
  m.def("tokens_to_chunk_hashes_fast", &kvidx::tokens_to_chunk_hashes_fast,
        py::arg("tokens"), py::arg("parent"), py::arg("block_size"),
        py::arg("algo") = 0);
  m.def("cpu_insert", &kvidx::cpu_insert);
  m.def("cpu_compact", &kvidx::cpu_compact);
  m.def("cpu_evict", &kvidx::cpu_evict);
  m.def("cpu_purge_pods", &kvidx::cpu_purge_pods);
  m.def("cpu_remap_pods", &kvidx::cpu_remap_pods);
  m.def("cpu_lookup", &kvidx::cpu_lookup);
  m.def("cpu_fused_score", &kvidx::cpu_fused_score);
  m.def("cpu_score_from_masks", &kvidx::cpu_score_from_masks);
  m.def("cpu_get_request_keys", &kvidx::cpu_get_request_keys);
#ifdef KVIDX_WITH_HIP
  m.attr("HAS_HIP") = true;
  m.def("gpu_insert", &kvidx::gpu_insert);
  m.def("gpu_compact", &kvidx::gpu_compact);
  m.def("gpu_evict", &kvidx::gpu_evict);
  // one launch; the GIL is released around it and the counter readback
  m.def("gpu_purge_pods", &kvidx::gpu_purge_pods,
        py::call_guard<py::gil_scoped_release>());
  m.def("gpu_remap_pods", &kvidx::gpu_remap_pods,
        py::call_guard<py::gil_scoped_release>());
  m.def("gpu_get_request_keys", &kvidx::gpu_get_request_keys);
  m.def("gpu_lookup", &kvidx::gpu_lookup);
  m.def("gpu_fused_score", &kvidx::gpu_fused_score);
  m.def("gpu_score_from_masks", &kvidx::gpu_score_from_masks);
  m.def("gpu_score_hashes", &kvidx::gpu_score_hashes);
  m.def("gpu_hash_chain", &kvidx::gpu_hash_chain,
        py::arg("tokens"), py::arg("tok_off"), py::arg("parents"),
        py::arg("block_size"), py::arg("algo") = 0);
  m.def("gpu_hash_chain_tr", &kvidx::gpu_hash_chain_tr,
        py::arg("tokens_t"), py::arg("parents"), py::arg("n_chunks"),
        py::arg("block_size"), py::arg("max_chunks"), py::arg("ilp") = 0,
        py::arg("row_major") = 0, py::arg("algo") = 0);
  m.def("gpu_fused_score_rows", &kvidx::gpu_fused_score_rows);
  m.def("gpu_stage_ragged_tokens", &kvidx::gpu_stage_ragged_tokens,
        py::arg("tokens"), py::arg("offsets"), py::arg("block_size"));
  // stage + chain + score in one call; the GIL is released for all of it
  m.def("gpu_score_flat_tokens", &kvidx::gpu_score_flat_tokens,
        py::arg("keys"), py::arg("meta"), py::arg("stamp"), py::arg("pods"),
        py::arg("e_keys"), py::arg("e_meta"), py::arg("e_vals"),
        py::arg("pods_per_key"), py::arg("tokens_flat"), py::arg("offsets"),
        py::arg("model_id"), py::arg("filter_words"), py::arg("weights"),
        py::arg("num_pods"), py::arg("epoch"), py::arg("init_hash_bits"),
        py::arg("block_size"), py::arg("n_tiers"), py::arg("algo") = 0,
        py::call_guard<py::gil_scoped_release>());
  m.def("gpu_apply_events", &kvidx::gpu_apply_events,
        py::arg("keys"), py::arg("meta"), py::arg("stamp"), py::arg("pods"),
        py::arg("e_keys"), py::arg("e_meta"), py::arg("e_vals"),
        py::arg("pods_per_key"), py::arg("tokens"), py::arg("tok_off"),
        py::arg("ehashes"), py::arg("eh_off"), py::arg("parents"),
        py::arg("has_parent"), py::arg("ev_type"), py::arg("pod_entry"),
        py::arg("grp_off"), py::arg("model_of"), py::arg("init_hash_bits"),
        py::arg("block_size"), py::arg("epoch"), py::arg("shard_id"),
        py::arg("num_shards"), py::arg("algo") = 0);
  m.def("gpu_apply_events_split", &kvidx::gpu_apply_events_split,
        py::arg("keys"), py::arg("meta"), py::arg("stamp"), py::arg("pods"),
        py::arg("e_keys"), py::arg("e_meta"), py::arg("e_vals"),
        py::arg("pods_per_key"), py::arg("tokens"), py::arg("tok_off"),
        py::arg("ehashes"), py::arg("eh_off"), py::arg("parents"),
        py::arg("has_parent"), py::arg("ev_type"), py::arg("pod_entry"),
        py::arg("grp_off"), py::arg("ev_of"), py::arg("model_of"),
        py::arg("init_hash_bits"), py::arg("block_size"), py::arg("epoch"),
        py::arg("shard_id"), py::arg("num_shards"), py::arg("algo") = 0);
  m.def("gpu_apply_events_split_tr", &kvidx::gpu_apply_events_split_tr,
        py::arg("keys"), py::arg("meta"), py::arg("stamp"), py::arg("pods"),
        py::arg("e_keys"), py::arg("e_meta"), py::arg("e_vals"),
        py::arg("pods_per_key"), py::arg("tokens_flat"), py::arg("tok_off"),
        py::arg("ehashes"), py::arg("eh_off"), py::arg("parents"),
        py::arg("has_parent"), py::arg("ev_type"), py::arg("pod_entry"),
        py::arg("ev_of"), py::arg("model_of"), py::arg("init_hash_bits"),
        py::arg("block_size"), py::arg("epoch"), py::arg("shard_id"),
        py::arg("num_shards"), py::arg("max_tokens"), py::arg("algo") = 0);
#else
  m.attr("HAS_HIP") = false;
#endif
  kvidx::wire::register_wirefront(m);
}
