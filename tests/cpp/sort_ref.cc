// TEST INFRASTRUCTURE: writes tests/golden/sort.json (run by
// tests/golden/make_sort.py): what std::stable_sort and std::unique give,
// with the reference's operator< (xdrpp/types.h:946-1062, XDRPP_STRONG_ORDER
// = 0), on a pool of 64 values of each genuine xdrc-generated type of
// tests/compare_fixture.py.  A pool holds seeded values from the generators
// of oracle/ (ref_objects.hh, xdrtest_gen.hh, workload_gen.h), copies of
// them with one seeded wire byte altered -- kept when xdr_from_opaque accepts
// them; they share long prefixes with their originals, so the deciding field
// wanders over the whole record -- for the float types NaN and signed-zero
// values, and exact duplicates of earlier members; then a seeded shuffle.
//
//   sort_ref OUT.json
#include <algorithm>
#include <cmath>
#include <compare>
#include <cstdio>
#include <functional>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "ref_objects.hh"
#include "xdrtest_gen.hh"

using std::string;
using std::vector;
using xdrtest_gen::rng;

namespace {

constexpr int kPool = 64, kSeeded = 28, kAltered = 16;

template <class B> string hex(const B &b) {
  static const char d[] = "0123456789abcdef";
  string s;
  const uint8_t *p = reinterpret_cast<const uint8_t *>(b.data());
  for (size_t i = 0; i < b.size(); ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
  return s;
}

struct writer {
  FILE *f;
  bool first_type = true;
};

void list(FILE *f, const char *key, const vector<int> &v) {
  fprintf(f, ",\"%s\":[", key);
  for (size_t i = 0; i < v.size(); ++i) fprintf(f, "%s%d", i ? "," : "", v[i]);
  fprintf(f, "]");
}

// `as`: seeded candidates (the first kSeeded go in as they are, the later
// ones are altered); specials: values the generators do not give.
template <class T>
void emit(writer &w, const char *name, bool has_float, const vector<T> &as, uint64_t seed, const vector<T> &specials) {
  vector<T> pool(as.begin(), as.begin() + kSeeded);
  rng g{seed};
  int tried = 0, dropped = 0;
  // one seeded byte of a candidate's encoding replaced; dropped when the reference refuses the bytes
  for (size_t i = kSeeded; int(pool.size()) < kSeeded + kAltered; ++i) {
    if (i >= as.size()) refobj::die(string(name) + ": out of candidates");
    // (mostly a copy of a pool member, so that the pool holds both sides)
    const T &from = g.below(4) ? pool[g.below(kSeeded)] : as[i];
    auto bytes = xdr::xdr_to_opaque(from);
    if (bytes.empty()) continue;
    ++tried;
    // the later of two draws (discriminants and counts, which rarely survive, come first); a
    // zero byte is padding, an absent pointer or the high bytes of a count, which the reference
    // refuses to see changed: drawn again
    size_t pos = 0;
    for (int t = 0; t < 8; ++t) {
      pos = std::max(g.below(uint32_t(bytes.size())), g.below(uint32_t(bytes.size())));
      if (bytes[pos]) break;
    }
    // payload bytes take any value; the low byte of a word (lengths, counts, discriminants,
    // bools, small enums) moves by one so that it often stays acceptable
    const uint8_t old = bytes[pos];
    uint8_t nv = uint8_t(g.below(256));
    if (pos % 4 == 3 && g.coin()) nv = uint8_t(old + (g.coin() ? 1 : -1));
    if (nv == old) nv = uint8_t(old ^ 1);
    bytes[pos] = nv;
    T b;
    try {
      xdr::xdr_from_opaque(bytes, b);
    } catch (const std::exception &) {
      ++dropped;
      continue;
    }
    pool.push_back(b);
  }
  if (2 * dropped > tried) refobj::die(string(name) + ": more than half of the altered candidates dropped");
  for (const auto &s : specials) pool.push_back(s);
  if (int(pool.size()) > kPool - 12) refobj::die(string(name) + ": no room for the duplicates");
  while (int(pool.size()) < kPool) pool.push_back(T(pool[g.below(uint32_t(pool.size()))]));
  for (size_t i = pool.size() - 1; i > 0; --i) std::swap(pool[i], pool[g.below(uint32_t(i + 1))]);

  vector<int> unsortable, sorted;
  for (int i = 0; i < kPool; ++i) (pool[i] == pool[i] ? sorted : unsortable).push_back(i);
  std::stable_sort(sorted.begin(), sorted.end(), [&](int a, int b) { return pool[a] < pool[b]; });
  vector<int> first;
  for (size_t k = 0; k < sorted.size(); ++k) first.push_back(k == 0 || pool[sorted[k - 1]] < pool[sorted[k]]);

  int repeats = 0;  // sortable values with an equivalent earlier pool member
  for (int i = 0; i < kPool; ++i) {
    if (!(pool[i] == pool[i])) continue;
    for (int j = 0; j < i; ++j)
      if (pool[j] == pool[j] && !(pool[j] < pool[i]) && !(pool[i] < pool[j])) { ++repeats; break; }
  }
  vector<int> ident(sorted), rev;
  std::sort(ident.begin(), ident.end());
  rev.assign(ident.rbegin(), ident.rend());
  if (sorted.size() < 48) refobj::die(string(name) + ": fewer than 48 sortable values");
  if (repeats < 8) refobj::die(string(name) + ": fewer than 8 values with an equivalent earlier one");
  if (sorted == ident || sorted == rev) refobj::die(string(name) + ": the pool is in order already");
  if (has_float && unsortable.size() < 2) refobj::die(string(name) + ": fewer than 2 unsortable values");

  fprintf(w.f, "%s\"%s\":{\"altered_tried\":%d,\"altered_dropped\":%d,\"values\":[", w.first_type ? "" : ",\n", name,
          tried, dropped);
  w.first_type = false;
  for (int i = 0; i < kPool; ++i) fprintf(w.f, "%s\"%s\"", i ? "," : "", hex(xdr::xdr_to_opaque(pool[i])).c_str());
  fprintf(w.f, "]");
  list(w.f, "unsortable", unsortable);
  list(w.f, "sorted", sorted);
  list(w.f, "first", first);
  fprintf(w.f, "}");
  fprintf(stderr, "%-16s %zu sortable, %d distinct, %d repeats, %zu unsortable; altered %d tried, %d dropped\n", name,
          sorted.size(), int(std::accumulate(first.begin(), first.end(), 0)), repeats, unsortable.size(), tried,
          dropped);
}

// NaNs (two bit patterns), a NaN behind an earlier differing field, both
// zeros and a number.
template <class T>
vector<T> float_specials(const T &base, const std::function<void(T &, double)> &setf,
                         const std::function<void(T &)> &earlier) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double nan2 = refobj::bits_as<double>(0xfff8000000001234ull);
  auto with = [&](double v) { T t = base; setf(t, v); return t; };
  T e = with(nan);
  earlier(e);
  return {with(nan), with(nan2), e, with(-0.0), with(0.0), with(1.5)};
}

uunion r_uunion(rng &g) {
  uunion u(1 + g.below(4));
  switch (u.d()) {
  case 1: u.one() = g.coin(); break;
  case 2: u.two() = int32_t(g.next()) >> g.below(28); break;
  case 3: u.three() = double(int32_t(g.next())) / 16.0; break;
  default: xdrtest_gen::rbytes(g, u.four(), 9); break;
  }
  return u;
}
uptr r_uptr(rng &g) {
  uptr u(g.below(12) != 0);  // (mostly with a value: its word is what an altered byte can move)
  if (u.b() && g.below(12)) u.val().activate() = int32_t(g.next()) >> g.below(28);
  return u;
}
testns::ContainsEnum r_contains(rng &g) {
  testns::ContainsEnum c(g.coin() ? RED : REDDER);
  if (c.c() == RED) xdrtest_gen::rbytes(g, c.foo(), 12);
  else c.num() = g.coin() ? testns::ContainsEnum::ONE : testns::ContainsEnum::TWO;
  return c;
}
template <class T, class F> vector<T> many(F &&f, uint64_t seed, int n) {
  rng g{seed};
  vector<T> v;
  for (int i = 0; i < n; ++i) v.push_back(f(g));
  return v;
}
void shrink(xdr::opaque_auth &a) { a.body.resize(a.body.size() % 41); }

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) refobj::die("usage: sort_ref OUT.json");
  writer w{fopen(argv[1], "w")};
  if (!w.f) refobj::die("cannot open output");
  const int N = 256;  // candidates per type
  fprintf(w.f, "{\"generator\":\"tests/cpp/sort_ref.cc: pools of 64 values (wire bytes); unsortable = the indices with "
               "!(x == x); sorted = std::stable_sort of the others by the reference's operator<; first[k] = k == 0 || "
               "v[sorted[k-1]] < v[sorted[k]]\",\n\"types\":{\n");
  {
    vector<testns::numerics> a;
    refobj::gen_numerics(N, 0x50A1, a);
    auto sp = float_specials<testns::numerics>(
        a[0], [](testns::numerics &t, double v) { t.f2 = v; }, [](testns::numerics &t) { t.i1 ^= 0x40; });
    auto sf = float_specials<testns::numerics>(
        a[1], [](testns::numerics &t, double v) { t.f1 = float(v); }, [](testns::numerics &t) { t.b = !t.b; });
    sp.insert(sp.end(), sf.begin(), sf.begin() + 2);
    emit(w, "numerics", true, a, 0x5171, sp);
  }
  {
    vector<rec128> a;
    refobj::gen_rec128(N, 0x50B1, 0, a);
    for (auto &x : a) {  // (random bit patterns may hold a NaN of their own)
      double *dd = &x.d0;
      for (int k = 0; k < 6; ++k)
        if (std::isnan(dd[k])) dd[k] = 0.25 * k;
    }
    auto sp = float_specials<rec128>(
        a[0], [](rec128 &t, double v) { t.d3 = v; }, [](rec128 &t) { t.u5 += 1; });
    emit(w, "rec128", true, a, 0x5172, sp);
  }
  {
    vector<recvar> a;
    refobj::gen_recvar(N, 0x50C1, a);
    for (auto &x : a) x.blob.resize(x.blob.size() % 65);  // (keeps the fixture small)
    auto sp = float_specials<recvar>(
        a[0], [](recvar &t, double v) { t.score = v; }, [](recvar &t) { t.name += "z"; });
    emit(w, "recvar", true, a, 0x5173, sp);
  }
  {
    vector<xdr::rpc_msg> a;
    refobj::gen_rpc(N, 0x50D1, a);
    for (auto &m : a)  // (keeps the fixture small: auth bodies of at most 40 bytes)
      if (m.body.mtype() == xdr::CALL) { shrink(m.body.cbody().cred); shrink(m.body.cbody().verf); }
    emit(w, "rpc_msg", false, a, 0x5174, {});
  }
  {
    auto a = many<uunion>(r_uunion, 0x50E1, N);
    uunion base(3);
    auto sp = float_specials<uunion>(
        base, [](uunion &t, double v) { t.three() = v; }, [](uunion &t) { t.d(2); t.two() = 7; });
    sp.erase(sp.begin() + 2);  // (the earlier field is the discriminant: that value holds no NaN)
    emit(w, "uunion", true, a, 0x5175, sp);
  }
  {
    auto a = many<uptr>(r_uptr, 0x50F1, N);
    emit(w, "uptr", false, a, 0x5176, {});
  }
  {
    auto a = many<testns::ContainsEnum>(r_contains, 0x5101, N);
    emit(w, "ContainsEnum", false, a, 0x5177, {});
  }
  {
    auto a = many<testns::containertest>(xdrtest_gen::r_containertest, 0x5111, N);
    testns::containertest base;
    base.uvec = {u_4_12(4), u_4_12(12), u_4_12(4)};
    base.uvec[1].f12().i = 3;
    base.sarr[0] = "hello";
    auto sp = float_specials<testns::containertest>(
        base, [](testns::containertest &t, double v) { t.uvec[1].f12().d = v; },
        [](testns::containertest &t) { t.uvec[0].f4().i = -1; });
    emit(w, "containertest", true, a, 0x5178, sp);
  }
  {
    auto a = many<testns::hasbytes>(xdrtest_gen::r_hasbytes, 0x5121, N);
    emit(w, "hasbytes", false, a, 0x5179, {});
  }
  {
    auto gen = [](rng &g) { return xdrtest_gen::r_recursive(g, 1 + int(g.below(2))); };
    auto a = many<test_recursive>(gen, 0x5131, N);
    emit(w, "test_recursive", false, a, 0x517A, {});
  }
  {
    vector<xdr::rp__list> a;
    refobj::gen_rp_list(N, 0x5141, a);
    emit(w, "rp__list", false, a, 0x517B, {});
  }
  fprintf(w.f, "\n}}\n");
  fclose(w.f);
  return 0;
}
