// host_xfer.h -- what sdmm_api.cpp defines for the runtime's other host
// translation units: the error slot, handle internals, and the host transfer
// and scratch helpers, whose rules are stated in sdmm_api.cpp ("Host transfer
// and scratch rules") and in DESIGN.md section 2 ("Concurrency").
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <mutex>

#include "../../include/sdmm_gpu.h"

namespace sdmm_detail {

// Sets the calling thread's error message (sdmm_last_error) and returns code.
int set_error(int code, const char* msg);

// sdmm_destroy (sync = false: the caller has synchronised the stream), and for
// n mixtures after one synchronisation per distinct stream.
void destroy_impl(sdmm_mix* m, bool sync);
void destroy_many(sdmm_mix* const* ms, int n);

// The tree's stream, with its device nodes uploaded (the device Li runs on it),
// and the device count of full-K (fallback) queries of its last guided call.
int tree_stream(sdmm_stree* t, hipStream_t* st);
const int* tree_fallback_count(const sdmm_stree* t);

// sdmm_push_training; reuse_counts: the call directly follows a count-only call
// with the same tree, paths, saved_per_path and seed, whose per-path record
// offsets in the tree's scratch are reused.  Without seg and lost nothing is
// read back: the call returns with the writes in flight on the tree's stream.
int push_training_ex(sdmm_stree* t, const sdmm_path_vertices* v, int saved_per_path, uint64_t seed,
                     const sdmm_training_out* out, int64_t* n_out, int64_t* seg, int64_t* lost, bool reuse_counts,
                     int64_t known_count);

// A device block grown on demand; owned by one (device, stream) pool entry.
struct StreamScratch {
    char* p = nullptr;
    size_t cap = 0;
};

// The calling thread's pinned bounce buffer of at least `bytes`.  Its previous
// contents are dead: every user synchronises its stream before it returns.
hipError_t bounce_buf(size_t bytes, char** out);

// The scratch entry of (device, stream), returned locked: hold the lock until
// the stream has been synchronised after the last use of the block.
std::unique_lock<std::mutex> stream_scratch(int device, hipStream_t st, StreamScratch** out);

// Grow s to at least `bytes` (the caller holds its lock, the stream is idle).
hipError_t scratch_reserve(StreamScratch& s, size_t bytes);

// Free every pool entry (sdmm_release_cached_scratch).
void release_stream_scratch();

}  // namespace sdmm_detail
