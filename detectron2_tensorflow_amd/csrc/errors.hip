// Thread-local host error string + the device error word (see include/d2mi.h).
#include <algorithm>
#include <climits>
#include <ctype.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "internal.h"

namespace {
thread_local char g_msg[1024] = "";
__device__ int32_t g_error_word = 0;
}  // namespace

namespace d2mi {

namespace {
#define X(id, key, def) key,
const char* const kTuneNames[kTuneCount] = {D2MI_TUNE_KNOBS(X)};
#undef X
#define X(id, key, def) def,
const int kTuneDefault[kTuneCount] = {D2MI_TUNE_KNOBS(X)};
#undef X
int g_tune[kTuneCount];
bool g_tune_set[kTuneCount];
}  // namespace

int tuning(TuneKey k) {
  if (!g_tune_set[k]) {
    std::string env = "D2MI_";  // + the key in capitals
    for (const char* c = kTuneNames[k]; *c; ++c) env += (char)toupper((unsigned char)*c);
    const char* e = getenv(env.c_str());
    g_tune[k] = e ? atoi(e) : kTuneDefault[k];
    g_tune_set[k] = true;
  }
  return g_tune[k];
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
  va_end(ap);
}

namespace {
__global__ void fill_u32_words_kernel(uint32_t* __restrict__ p, size_t n, uint32_t v) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}
__global__ void fill_u8_kernel(uint8_t* __restrict__ p, size_t n, uint8_t v) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = v;
}
}  // namespace

// A byte fill as a kernel on ``st`` (in place of hipMemsetAsync, r5): inside
// a captured hipGraph a memset becomes a memset node, and the graphed
// training step's replays diverged from the eager step only where a buffer
// zeroed by one fed an atomic accumulation (the matcher's per-GT best IoU)
// and only when the batch changed -- the node's ordering against the
// kernels around it is not what the stream order was.  A kernel node is
// ordered like every other launch of the capture.
int fill_bytes(void* p, size_t nbytes, uint8_t value, hipStream_t st) {
  if (nbytes == 0) return 0;
  if (((uintptr_t)p & 3) == 0 && (nbytes & 3) == 0) {
    const size_t n = nbytes / 4;
    const uint32_t v = 0x01010101u * value;
    hipLaunchKernelGGL(fill_u32_words_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)),
                       dim3(256), 0, st, (uint32_t*)p, n, v);
  } else {
    hipLaunchKernelGGL(fill_u8_kernel, dim3((unsigned)std::min<size_t>((nbytes + 255) / 256, 4096)),
                       dim3(256), 0, st, (uint8_t*)p, nbytes, value);
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int32_t* error_word() {
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_error_word)) != hipSuccess) return nullptr;
  return (int32_t*)p;
}

}  // namespace d2mi

extern "C" {

int d2mi_version(void) { return 1; }

// Hash of the sources this library was built from (csrc/*.hip, csrc/*.h,
// include/d2mi.h; _build.source_hash), passed in by the build: _C.load
// refuses a library whose hash differs from the tree it is loaded from.
#ifndef D2MI_SOURCE_HASH
#define D2MI_SOURCE_HASH "unknown"
#endif
const char* d2mi_source_hash(void) { return D2MI_SOURCE_HASH; }

const char* d2mi_last_error(void) { return g_msg; }

int d2mi_set_tuning(const char* key, int value) {
  D2MI_REQUIRE(key != nullptr, "null tuning key");
  for (int k = 0; k < d2mi::kTuneCount; ++k) {
    if (strcmp(key, d2mi::kTuneNames[k]) == 0) {
      d2mi::g_tune[k] = value;
      d2mi::g_tune_set[k] = true;
      return 0;
    }
  }
  D2MI_REQUIRE(false, "unknown tuning key '%s'", key);
  return -1;
}

int d2mi_get_tuning(const char* key) {
  if (key == nullptr) return INT32_MIN;
  for (int k = 0; k < d2mi::kTuneCount; ++k)
    if (strcmp(key, d2mi::kTuneNames[k]) == 0) return d2mi::tuning((d2mi::TuneKey)k);
  return INT32_MIN;
}

int32_t* d2mi_error_word_dev(void) { return d2mi::error_word(); }

// Node census of a captured (not yet instantiated) hipGraph: counts[t] = the
// number of nodes of hipGraphNodeType t, for t < ntypes.  The graphed
// training step (engine/graphed.py) refuses a capture holding memset nodes
// while the runtime's graph packet capture is on: those are the nodes whose
// order against the kernels around them it does not keep (r5).
int d2mi_graph_census(void* graph, long long* counts, int ntypes) {
  D2MI_REQUIRE(graph != nullptr && counts != nullptr && ntypes > 0, "bad graph census arguments");
  for (int t = 0; t < ntypes; ++t) counts[t] = 0;
  size_t n = 0;
  D2MI_REQUIRE(hipGraphGetNodes((hipGraph_t)graph, nullptr, &n) == hipSuccess,
               "hipGraphGetNodes failed");
  if (n == 0) return 0;
  hipGraphNode_t* nodes = (hipGraphNode_t*)malloc(n * sizeof(hipGraphNode_t));
  D2MI_REQUIRE(nodes != nullptr, "out of host memory");
  int rc = 0;
  if (hipGraphGetNodes((hipGraph_t)graph, nodes, &n) != hipSuccess) {
    d2mi::set_error("hipGraphGetNodes failed");
    rc = -1;
  }
  for (size_t i = 0; rc == 0 && i < n; ++i) {
    hipGraphNodeType t;
    if (hipGraphNodeGetType(nodes[i], &t) != hipSuccess) {
      d2mi::set_error("hipGraphNodeGetType failed");
      rc = -1;
    } else if ((int)t >= 0 && (int)t < ntypes) {
      ++counts[(int)t];
    }
  }
  free(nodes);
  return rc;
}

// The same census of the graph a stream is capturing into right now (a
// diagnosis: tools/graph_nodes.py runs it after every op of a capture to name
// the ops that add memset / memcpy nodes).  Returns 1 when the stream is not
// capturing (counts all 0).
int d2mi_capture_census(void* stream, long long* counts, int ntypes) {
  D2MI_REQUIRE(counts != nullptr && ntypes > 0, "bad capture census arguments");
  for (int t = 0; t < ntypes; ++t) counts[t] = 0;
  hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  hipGraph_t graph = nullptr;
  const hipGraphNode_t* deps = nullptr;
  size_t ndeps = 0;
  D2MI_REQUIRE(hipStreamGetCaptureInfo_v2(d2mi::as_stream(stream), &status, &id, &graph, &deps,
                                          &ndeps) == hipSuccess,
               "hipStreamGetCaptureInfo_v2 failed");
  if (status != hipStreamCaptureStatusActive || graph == nullptr) return 1;
  return d2mi_graph_census((void*)graph, counts, ntypes);
}

int d2mi_clear_errors(void* stream) {
  int32_t* w = d2mi::error_word();
  D2MI_REQUIRE(w != nullptr, "cannot resolve the device error word");
  D2MI_REQUIRE(d2mi::fill_bytes(w, sizeof(int32_t), 0, d2mi::as_stream(stream)) == 0,
               "error word clear failed");
  return 0;
}

}  // extern "C"
