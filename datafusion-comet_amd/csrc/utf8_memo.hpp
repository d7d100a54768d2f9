// The length a previous task VERIFIED for an undeclared, unsliced Utf8 column of a device input, process-wide, keyed by (plan hash, input index,
// column).  It is a guess about which variant of the fused kernel to launch before the column's offsets have been read — never a verdict: every
// task still checks every offset (exec_input.cpp / exec_pipeline.cpp), and a task whose check disagrees forgets the entry.
// Bounded and mutex-guarded like the verdict cache of declared columns next to its use; header-only and free of the executor's types, so a
// stand-alone program can exercise it from several threads (tests/utf8_memo_host).
#ifndef COMET_UTF8_MEMO_HPP
#define COMET_UTF8_MEMO_HPP

#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>

namespace comet {

class Utf8LengthMemo {
 public:
  explicit Utf8LengthMemo(size_t max_entries = 4096) : max_(max_entries) {}
  // → true and the remembered length
  bool get(uint64_t plan_hash, size_t input, size_t column, int& len) const {
    std::lock_guard<std::mutex> g(mu_);
    auto it = map_.find(Key{plan_hash, input, column});
    if (it == map_.end()) return false;
    len = it->second;
    return true;
  }
  void put(uint64_t plan_hash, size_t input, size_t column, int len) {
    std::lock_guard<std::mutex> g(mu_);
    if (map_.size() >= max_ && map_.find(Key{plan_hash, input, column}) == map_.end()) map_.clear();      // bounded; cleared when full
    map_[Key{plan_hash, input, column}] = len;
  }
  void forget(uint64_t plan_hash, size_t input, size_t column) {
    std::lock_guard<std::mutex> g(mu_);
    map_.erase(Key{plan_hash, input, column});
  }
  size_t size() const {
    std::lock_guard<std::mutex> g(mu_);
    return map_.size();
  }

 private:
  typedef std::tuple<uint64_t, size_t, size_t> Key;
  const size_t max_;
  mutable std::mutex mu_;
  std::map<Key, int> map_;
};

}  // namespace comet

#endif
