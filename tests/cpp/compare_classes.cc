// TEST INFRASTRUCTURE (tests/test_compare_classes_cpp.py): the value classes
// include/xdrpp_gpu.hh records beside the plan ops of the reference's
// genuine xdrc-generated types, printed op for op:
//
//   type NAME NOPS
//   KIND CLASS        (one line per op)
//
// and xdr::gpu::compare_batch instantiated for each of them (not run: this
// program never touches a device).
#include <cstdio>

#include "ref_types.hh"
#include "xdrpp_gpu.hh"

template <typename T> void dump(const char *name) {
  const xdr::gpu::recorded_plan<T> p;
  if (p.compare_classes.size() != p.ops.size()) {
    std::fprintf(stderr, "%s: %zu classes for %zu ops\n", name, p.compare_classes.size(), p.ops.size());
    std::exit(1);
  }
  std::printf("type %s %zu\n", name, p.ops.size());
  for (std::size_t i = 0; i < p.ops.size(); ++i) std::printf("%u %u\n", p.ops[i].kind, p.compare_classes[i]);
  // the wrapper over xdrg_compare compiles for T
  void (*f)(const void *, const void *, std::uint64_t, const void *, const void *, std::uint64_t, std::uint64_t,
            std::int8_t *, hipStream_t) = &xdr::gpu::compare_batch<T>;
  if (!f) std::exit(1);
}

int main() {
  dump<testns::numerics>("numerics");
  dump<rec128>("rec128");
  dump<recvar>("recvar");
  dump<xdr::rpc_msg>("rpc_msg");
  dump<uunion>("uunion");
  dump<uptr>("uptr");
  dump<testns::ContainsEnum>("ContainsEnum");
  dump<testns::containertest>("containertest");
  dump<testns::hasbytes>("hasbytes");
  dump<test_recursive>("test_recursive");
  dump<xdr::rp__list>("rp__list");
  return 0;
}
