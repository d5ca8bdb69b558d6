// TEST INFRASTRUCTURE (tests/test_sort_batch_cpp.py): xdr::gpu::sort_batch
// and sort_workspace_size instantiated for genuine xdrc-generated types of
// the reference, and their host-check paths called: a null argument throws
// the XDRG_EINVAL exception, n = 0 returns.  This program never touches a
// device.  Prints "ok NAME" per type.
#include <cstdio>
#include <cstdlib>
#include <exception>

#include "ref_types.hh"
#include "xdrpp_gpu.hh"

template <typename T> void check(const char *name) {
  const std::size_t w1 = xdr::gpu::sort_workspace_size<T>(1), w2 = xdr::gpu::sort_workspace_size<T>(100000);
  if (!w1 || w2 < w1) {
    std::fprintf(stderr, "%s: workspace sizes %zu, %zu\n", name, w1, w2);
    std::exit(1);
  }
  // n = 0: launches nothing, needs nothing
  xdr::gpu::sort_batch<T>(nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, 0);
  // n = 1 without records: refused by the host checks
  alignas(16) static unsigned char fake[64];  // (never dereferenced)
  bool threw = false;
  try {
    xdr::gpu::sort_batch<T>(nullptr, nullptr, 0, 1, reinterpret_cast<std::uint32_t *>(fake), nullptr,
                            reinterpret_cast<std::uint64_t *>(fake), fake, w1);
  } catch (const xdr::gpu::api_error &e) {
    threw = e.code == XDRG_EINVAL;
    std::printf("refused %s: %s\n", name, e.what());
  }
  if (!threw) {
    std::fprintf(stderr, "%s: a null batch was accepted\n", name);
    std::exit(1);
  }
  std::printf("ok %s\n", name);
}

int main() {
  check<testns::numerics>("numerics");
  check<testns::containertest>("containertest");
  check<xdr::rp__list>("rp__list");
  return 0;
}
