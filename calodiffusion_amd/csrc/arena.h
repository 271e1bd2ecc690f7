// The workspace allocator of the plan's launch sequences.
#pragma once
#include "../../include/calodiff.h"
#include "cd_common.h"

#include <vector>

namespace cd {

// ------------------------------------------------------------------------------------------------------------
// workspace allocator: deterministic first-fit over the caller's workspace, replayed identically by a dry run
// (to size the workspace) and by every real call (so captured graphs see stable addresses).
// ------------------------------------------------------------------------------------------------------------
class Arena {
 public:
  void reset(char* base, size_t cap, bool dry) {
    base_ = base; cap_ = cap; dry_ = dry; high_ = 0;
    blocks_.clear();
    blocks_.push_back({0, (size_t)1 << 60, true});
  }
  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    for (size_t i = 0; i < blocks_.size(); ++i) {
      if (blocks_[i].free && blocks_[i].size >= bytes) {
        const size_t off = blocks_[i].off;
        if (blocks_[i].size > bytes) {
          Block rest{off + bytes, blocks_[i].size - bytes, true};
          blocks_[i].size = bytes;
          blocks_.insert(blocks_.begin() + i + 1, rest);
        }
        blocks_[i].free = false;
        if (off + bytes > high_) high_ = off + bytes;
        if (!dry_ && off + bytes > cap_) throw Fail{CD_EWORKSPACE, "workspace too small: call cd_plan_workspace_bytes for this batch size"};
        return dry_ ? (void*)(uintptr_t)(0x1000 + off) : (void*)(base_ + off);
      }
    }
    throw Fail{CD_EWORKSPACE, "workspace allocator exhausted"};
  }
  template <typename T>
  T* get(size_t count) { return (T*)alloc(count * sizeof(T)); }
  void release(const void* p) {
    if (!p) return;
    const size_t off = dry_ ? (size_t)((uintptr_t)p - 0x1000) : (size_t)((const char*)p - base_);
    for (size_t i = 0; i < blocks_.size(); ++i) {
      if (blocks_[i].off == off && !blocks_[i].free) {
        blocks_[i].free = true;
        if (i + 1 < blocks_.size() && blocks_[i + 1].free) {
          blocks_[i].size += blocks_[i + 1].size;
          blocks_.erase(blocks_.begin() + i + 1);
        }
        if (i > 0 && blocks_[i - 1].free) {
          blocks_[i - 1].size += blocks_[i].size;
          blocks_.erase(blocks_.begin() + i);
        }
        return;
      }
    }
    throw Fail{CD_EINVAL, "internal: release of unknown workspace block"};
  }
  size_t high() const { return high_; }
  bool dry() const { return dry_; }

 private:
  struct Block { size_t off, size; bool free; };
  std::vector<Block> blocks_;
  char* base_ = nullptr;
  size_t cap_ = 0, high_ = 0;
  bool dry_ = false;
};

}  // namespace cd
