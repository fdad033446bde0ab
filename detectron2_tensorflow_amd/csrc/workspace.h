// Caller-owned workspaces: the bump allocator and its sizing twin (host-only
// header: no HIP types).
#pragma once
#include <stddef.h>

namespace d2mi {

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over a caller-owned workspace.
struct Workspace {
  char* base;
  size_t cap;
  size_t off;
  Workspace(void* b, size_t c) : base((char*)b), cap(c), off(0) {}
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    T* p = (T*)(base + off);
    off += n * sizeof(T);
    return p;
  }
  bool ok() const { return off <= cap; }
};

// Sizing twin of Workspace (same alignment rule, null pointers): a layout
// written once as a template over the allocator is carved over a Workspace
// by the op and measured over a WorkspaceSizer by its *_workspace_size().
struct WorkspaceSizer {
  size_t off = 0;
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    off += n * sizeof(T);
    return nullptr;
  }
};

// Bytes of a layout struct L { template <typename A> void lay(A&, args...); }.
template <typename L, typename... Args>
size_t layout_bytes(const Args&... args) {
  L l;
  WorkspaceSizer z;
  l.lay(z, args...);
  return z.off;
}

}  // namespace d2mi
