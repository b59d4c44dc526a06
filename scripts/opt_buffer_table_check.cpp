// Stand-alone check of the two HOST functions of the buffer table (include/avmoe.h: avmoe_opt_buffer_table_bytes, avmoe_opt_buffer_table_build)
// under AddressSanitizer and UndefinedBehaviorSanitizer: the image is built into a heap block of EXACTLY the bytes asked for (and once more at
// an address that is only 1-byte aligned), so a write past the image or a misaligned store is reported.  No GPU is touched: nothing is launched.
// Build and run from the repository root (host code only is instrumented):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         scripts/opt_buffer_table_check.cpp avmoe_amd/csrc/opt_kernels.hip avmoe_amd/csrc/common.cpp -o avmoe_amd/lib/variants/opt_buffer_table_check
//   avmoe_amd/lib/variants/opt_buffer_table_check
// Exit status 0 and "ok" on the last line: every image had the expected block map and no sanitizer report was raised.
#include "../include/avmoe.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace avmoe { const char* last_error(); }    // csrc/common.cpp: what avmoe_last_error (csrc/capi.cpp, not linked here) returns

static int fail(const char* what) {
  const char* e = avmoe::last_error();
  std::fprintf(stderr, "FAILED: %s (%s)\n", what, e ? e : "");
  return 1;
}

static int check(const std::vector<int64_t>& lengths, size_t misalign) {
  // the addresses are never dereferenced by the table functions: any 4-byte / 16-byte aligned values serve
  std::vector<avmoe_opt_buffer> recs(lengths.size());
  for (size_t i = 0; i < lengths.size(); ++i) recs[i] = avmoe_opt_buffer{(float*)(uintptr_t)(0x10000 + 64 * i + 4), (float*)(uintptr_t)(0x80000 + 16 * i), lengths[i]};
  int64_t nb = -1, want = 0;
  for (int64_t n : lengths) want += (n + 1023) / 1024;
  const size_t bytes = avmoe_opt_buffer_table_bytes(recs.data(), (int32_t)recs.size(), &nb);
  if (bytes == 0 || nb != want || bytes % 16 != 0) return fail("avmoe_opt_buffer_table_bytes");
  char* block = (char*)std::malloc(bytes + misalign);       // exactly the image: ASan guards the byte behind it
  if (!block) return fail("malloc");
  char* image = block + misalign;
  if (avmoe_opt_buffer_table_build(recs.data(), (int32_t)recs.size(), image, bytes) != 0) { std::free(block); return fail("avmoe_opt_buffer_table_build"); }
  int32_t n_buffers; int64_t n_blocks;
  std::memcpy(&n_buffers, image + 4, 4);
  std::memcpy(&n_blocks, image + 8, 8);
  int bad = (n_buffers != (int32_t)recs.size()) || (n_blocks != want);
  const char* map = image + 16 + sizeof(avmoe_opt_buffer) * recs.size();
  int64_t b = 0;
  for (size_t i = 0; i < lengths.size() && !bad; ++i)
    for (int64_t k = 0; k < (lengths[i] + 1023) / 1024; ++k, ++b) {
      int32_t pair[2];
      std::memcpy(pair, map + 8 * b, 8);
      if (pair[0] != (int32_t)i || pair[1] != (int32_t)k) bad = 1;
    }
  // one byte too few is refused before anything is written
  if (!bad && bytes > 16 && avmoe_opt_buffer_table_build(recs.data(), (int32_t)recs.size(), image, bytes - 1) != AVMOE_ERR_WORKSPACE) bad = 1;
  std::free(block);
  if (bad) return fail("the image's header or block map");
  std::printf("lengths %zu, misaligned by %zu: %lld blocks, %zu bytes\n", lengths.size(), misalign, (long long)nb, bytes);
  return 0;
}

int main() {
  const std::vector<int64_t> api = {1, 1024, 1025, 2049};                                    // the lengths of the table-image test
  const std::vector<int64_t> gpu = {1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049};           // the lengths of the GPU test
  const std::vector<int64_t> edge = {0, 5, 0};
  int rc = 0;
  for (size_t misalign : {(size_t)0, (size_t)1}) {
    rc |= check(api, misalign);
    rc |= check(gpu, misalign);
    rc |= check(edge, misalign);
    rc |= check({}, misalign);
  }
  // refused lists: no write, no read past the list
  avmoe_opt_buffer r{(float*)(uintptr_t)0x10002, (float*)(uintptr_t)0x80000, 4};
  char img[64];
  if (avmoe_opt_buffer_table_build(&r, 1, img, sizeof img) != AVMOE_ERR_ALIGNMENT) rc |= fail("a 2-byte aligned buffer was accepted");
  if (avmoe_opt_buffer_table_build(&r, -1, img, sizeof img) != AVMOE_ERR_BAD_ARG) rc |= fail("a negative count was accepted");
  if (avmoe_opt_buffer_table_bytes(nullptr, 3, nullptr) != 0) rc |= fail("a NULL list was accepted");
  std::puts(rc ? "FAILED" : "ok");
  return rc;
}
