// Stand-alone exerciser of csrc/utf8_memo.hpp: eight threads get / put / forget overlapping keys of a small, bounded memo while it fills up and is
// cleared.  Built with -fsanitize=address,undefined by tests/test_utf8_memo_cpu.py and run on the CPU; prints "ok" and exits 0 when every answer was
// one a thread could have put.
#include <cstdio>
#include <thread>
#include <vector>

#include "utf8_memo.hpp"

int main() {
  comet::Utf8LengthMemo memo(64);
  // single-threaded contract first
  int len = -1;
  if (memo.get(1, 0, 4, len)) return 2;
  memo.put(1, 0, 4, 1);
  if (!memo.get(1, 0, 4, len) || len != 1) return 3;
  if (memo.get(1, 0, 5, len) || memo.get(1, 1, 4, len) || memo.get(2, 0, 4, len)) return 4;      // every part of the key counts
  memo.put(1, 0, 4, 7);
  if (!memo.get(1, 0, 4, len) || len != 7 || memo.size() != 1) return 5;
  memo.forget(1, 0, 4);
  memo.forget(1, 0, 4);
  if (memo.get(1, 0, 4, len) || memo.size() != 0) return 6;
  for (int k = 0; k < 1000; k++) memo.put(9, 0, (size_t)k, k & 15);
  if (memo.size() > 64) return 7;                                                                   // bounded
  if (!memo.get(9, 0, 999, len) || len != (999 & 15)) return 8;                                     // the newest entry survives a clear

  std::vector<int> bad(8, 0);
  std::vector<std::thread> threads;
  for (int t = 0; t < 8; t++)
    threads.emplace_back([&memo, &bad, t] {
      for (int i = 0; i < 20000; i++) {
        const uint64_t plan = (uint64_t)(i % 5);
        const size_t input = (size_t)(i % 2), col = (size_t)((i * 7 + t) % 24);
        switch ((i + t) % 4) {
          case 0: memo.put(plan, input, col, (int)(col % 16)); break;       // the length is a function of the key: any answer can be checked
          case 1: memo.forget(plan, input, col); break;
          default: {
            int got = -1;
            if (memo.get(plan, input, col, got) && got != (int)(col % 16)) bad[(size_t)t]++;
          }
        }
        if (memo.size() > 64) bad[(size_t)t]++;
      }
    });
  for (auto& th : threads) th.join();
  for (int b : bad)
    if (b) return 9;
  puts("ok");
  return 0;
}
