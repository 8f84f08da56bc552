// Host-side check of the hub-row workspace of ragraph_amd/csrc/sparse.hip, stand-alone (no device, no Python): the two size
// entries over a table of arguments against their closed forms, and long_rows_layout on a heap buffer of EXACTLY the size it
// reported -- every piece inside the buffer, 256-byte aligned relative to it, no two pieces overlapping, first and last byte
// of every piece written (under the host AddressSanitizer a piece that leaves the buffer is a report).
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -I include -I ragraph_amd/csrc \
//         tools/check_sparse_layout.hip -o /tmp/check_sparse_layout && /tmp/check_sparse_layout
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "sparse.hip"

namespace ragraph {
void set_error(const char* fmt, ...) {   // (the library's lives in rowops.hip)
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
}  // namespace ragraph

static size_t a(size_t x) { return (x + 255) / 256 * 256; }
static int failures = 0;
#define EXPECT(cond, ...)            \
  do {                               \
    if (!(cond)) {                   \
      ++failures;                    \
      printf("FAILED: " __VA_ARGS__); \
      printf("\n");                  \
    }                                \
  } while (0)

// Lays the area out on a buffer of exactly `bytes` and checks the pieces.
static void check_pieces(LongRowsCapacity cap, int partial_floats, int64_t request_slots, size_t bytes) {
  if (bytes > ((size_t)256 << 20)) return;   // (the sizes above are checked by their closed form only)
  char* buf = static_cast<char*>(malloc(bytes));
  LongRows w{};
  int* slot = nullptr;
  const size_t got = long_rows_layout(cap, partial_floats, request_slots, buf, &w, &slot);
  EXPECT(got == bytes, "layout on a buffer reports %zu, without one %zu", got, bytes);
  EXPECT(w.max_rows == cap.max_rows && w.max_tasks == cap.max_tasks, "capacity not passed on");
  EXPECT((slot != nullptr) == (request_slots > 0), "slot piece");
  std::vector<std::pair<char*, size_t>> pieces = {
      {reinterpret_cast<char*>(w.ctr), 2 * sizeof(int)},
      {reinterpret_cast<char*>(w.rows), (size_t)cap.max_rows * sizeof(int64_t)},
      {reinterpret_cast<char*>(w.pos), (size_t)cap.max_rows * sizeof(int)},
      {reinterpret_cast<char*>(w.task_row), (size_t)cap.max_tasks * sizeof(int64_t)},
      {reinterpret_cast<char*>(w.task_blk), (size_t)cap.max_tasks * sizeof(int)},
      {reinterpret_cast<char*>(w.partial), (size_t)cap.max_tasks * (size_t)partial_floats * sizeof(float)}};
  if (slot) pieces.push_back({reinterpret_cast<char*>(slot), (size_t)request_slots * sizeof(int)});
  std::sort(pieces.begin(), pieces.end());
  for (size_t i = 0; i < pieces.size(); ++i) {
    char* p = pieces[i].first;
    const size_t len = pieces[i].second;
    EXPECT(p >= buf && p + len <= buf + bytes, "piece %zu leaves the buffer", i);
    EXPECT((size_t)(p - buf) % 256 == 0, "piece %zu is not on a multiple of 256 bytes", i);
    EXPECT(i + 1 == pieces.size() || p + len <= pieces[i + 1].first, "pieces %zu and %zu overlap", i, i + 1);
    p[0] = 1;
    p[len - 1] = 2;
  }
  free(buf);
}

int main() {
  const int64_t NNZ[] = {0, 4095, 4096, 4097, 123457, 44000000};
  const int DS[] = {0, 4, 64, 256};
  const int64_t RS[] = {0, 1, 7, 6144, 4000000};
  long checked = 0;
  for (int64_t nnz : NNZ) {
    const size_t q = (size_t)(nnz / 4096);
    for (int D : DS) {
      const size_t mr = q + 1, mt = 2 * q + 2, d = D > 0 ? D : 1;
      const size_t want = a(8) + a(8 * mr) + a(4 * mr) + a(8 * mt) + a(4 * mt) + a(4 * mt * d);
      const size_t got = ragraph_sparse_workspace_bytes(nnz, D);
      EXPECT(got == want, "sparse_workspace_bytes(%lld, %d) = %zu, closed form %zu", (long long)nnz, D, got, want);
      check_pieces(full_capacity(nnz), (int)d, 0, got);
      ++checked;
      if (D < 1) continue;
      for (int64_t R : RS) {
        const size_t t = (size_t)R + q + 1, r = t / 2 + 1;
        const size_t want_r = a(8) + a(4 * (size_t)(R > 0 ? R : 1)) + a(8 * r) + a(4 * r) + a(8 * t) + a(4 * t) + a(4 * t * D);
        const size_t got_r = ragraph_spmm_csr_rows_workspace_bytes(nnz, R, D);
        EXPECT(got_r == want_r, "spmm_csr_rows_workspace_bytes(%lld, %lld, %d) = %zu, closed form %zu", (long long)nnz,
               (long long)R, D, got_r, want_r);
        check_pieces(subset_capacity(nnz, R), D, R > 0 ? R : 1, got_r);
        ++checked;
      }
    }
  }
  EXPECT(ragraph_sparse_workspace_bytes(-1, 64) == 0 && ragraph_sparse_workspace_bytes(4097, -1) == 0, "bad input: not 0");
  EXPECT(ragraph_spmm_csr_rows_workspace_bytes(-1, 7, 64) == 0 && ragraph_spmm_csr_rows_workspace_bytes(4097, -1, 64) == 0 &&
             ragraph_spmm_csr_rows_workspace_bytes(4097, 7, 0) == 0, "bad input: not 0 (rows)");
  EXPECT(ragraph_spmm_csr_rows_workspace_bytes(0, (int64_t)INT_MAX - 1, 4) == 0 &&
             ragraph_spmm_csr_rows_workspace_bytes(0, (int64_t)INT_MAX - 2, 4) != 0, "the int32 guard moved");
  printf("%ld argument sets checked, %d failures\n", checked, failures);
  return failures ? 1 : 0;
}
