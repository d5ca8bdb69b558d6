// TEST INFRASTRUCTURE: writes tests/golden/compare.json (run by
// tests/golden/make_compare.py): what the reference's operator<=> and
// operator== (xdrpp/types.h:946-1062, XDRPP_STRONG_ORDER = 0) give seeded
// pairs of the genuine xdrc-generated types.  a comes from the seeded
// generators of oracle/ (ref_objects.hh, xdrtest_gen.hh, workload_gen.h); b
// is a again, an independent value, or a's wire bytes with one seeded byte
// altered -- kept when xdr_from_opaque accepts them, so the deciding field
// wanders over the whole record.  Float types add NaN and signed-zero pairs.
//
//   compare_ref OUT.json
#include <algorithm>
#include <cmath>
#include <compare>
#include <cstdio>
#include <functional>
#include <limits>
#include <string>
#include <vector>

#include "ref_objects.hh"
#include "xdrtest_gen.hh"

using std::string;
using std::vector;
using xdrtest_gen::rng;

namespace {

constexpr int kEach = 22;  // pairs of each kind (same / independent / altered) per type

int ord(std::partial_ordering c) {
  return c == std::partial_ordering::less ? -1 : c == std::partial_ordering::equivalent ? 0
         : c == std::partial_ordering::greater ? 1 : 2;
}
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

template <class T> struct pair_t {
  T a, b;
  string b_hex;  // altered pairs: "@pos=byte", the one byte of a's encoding that b's differs in (else empty)
  const char *how;
};

template <class T>
void emit(writer &w, const char *name, bool has_float, const vector<T> &as, const vector<T> &others,
          uint64_t seed, const vector<pair_t<T>> &specials) {
  vector<pair_t<T>> ps;
  for (int i = 0; i < kEach; ++i) ps.push_back({as[i], as[i], "", "same"});
  for (int i = 0; i < kEach; ++i) ps.push_back({as[kEach + i], others[i], "", "indep"});
  // one seeded byte of a's encoding replaced; dropped when the reference refuses the bytes
  rng g{seed};
  int tried = 0, dropped = 0;
  for (size_t i = 2 * kEach; int(ps.size()) < 3 * kEach; ++i) {
    if (i >= as.size()) refobj::die(string(name) + ": out of candidates");
    auto bytes = xdr::xdr_to_opaque(as[i]);
    if (bytes.empty()) continue;
    ++tried;
    // (the later of two draws: discriminants and counts, which rarely survive, come first)
    // and a zero byte is padding, an absent pointer or the high bytes of a count, which the
    // reference refuses to see changed: drawn again)
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
    char where[32];  // b = a's bytes with byte `pos` set to `nv`
    snprintf(where, sizeof where, "@%zu=%02x", pos, unsigned(nv));
    ps.push_back({as[i], b, where, "alter"});
  }
  if (2 * dropped > tried) refobj::die(string(name) + ": more than half of the altered candidates dropped");
  for (const auto &s : specials) ps.push_back(s);

  int cnt[4] = {0, 0, 0, 0};
  fprintf(w.f, "%s\"%s\":{\"altered_tried\":%d,\"altered_dropped\":%d,\"pairs\":[", w.first_type ? "" : ",\n", name,
          tried, dropped);
  w.first_type = false;
  for (size_t i = 0; i < ps.size(); ++i) {
    const auto &p = ps[i];
    const int c = ord(p.a <=> p.b);
    const bool eq = p.a == p.b;
    ++cnt[c + 1];
    const string ha = hex(xdr::xdr_to_opaque(p.a));
    const string hb = !strcmp(p.how, "same") ? string() : p.b_hex.empty() ? hex(xdr::xdr_to_opaque(p.b)) : p.b_hex;
    fprintf(w.f, "%s[\"%s\",\"%s\",\"%s\",%d,%d]", i ? "," : "", p.how, ha.c_str(), hb.c_str(), c, eq ? 1 : 0);
  }
  fprintf(w.f, "]}");
  if (ps.size() < 64) refobj::die(string(name) + ": fewer than 64 pairs");
  for (int k = 0; k < 3; ++k)
    if (cnt[k] < 4) refobj::die(string(name) + ": a result appears fewer than 4 times");
  if (has_float && cnt[3] < 4) refobj::die(string(name) + ": unordered appears fewer than 4 times");
  fprintf(stderr, "%-16s %3zu pairs: less %d equal %d greater %d unordered %d; altered %d tried, %d dropped\n", name,
          ps.size(), cnt[0], cnt[1], cnt[2], cnt[3], tried, dropped);
}

// NaN against itself, against a number (both ways), other NaN patterns,
// -0.0 against +0.0, and a NaN behind an earlier differing field.
template <class T>
vector<pair_t<T>> float_specials(const T &base, const std::function<void(T &, double)> &setf,
                                 const std::function<void(T &)> &earlier) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double nan2 = refobj::bits_as<double>(0xfff8000000001234ull);
  auto with = [&](double v) { T t = base; setf(t, v); return t; };
  vector<pair_t<T>> s;
  s.push_back({with(nan), with(nan), "", "special"});
  s.push_back({with(nan), with(1.5), "", "special"});
  s.push_back({with(-2.0), with(nan), "", "special"});
  s.push_back({with(nan2), with(nan), "", "special"});
  s.push_back({with(nan2), with(nan2), "", "special"});
  s.push_back({with(-0.0), with(0.0), "", "special"});
  s.push_back({with(0.0), with(-0.0), "", "special"});
  T e = with(nan);
  earlier(e);
  s.push_back({with(nan), e, "", "special"});
  s.push_back({e, with(nan), "", "special"});
  return s;
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
void shrink(vector<xdr::rpc_msg> &v) {  // (keeps the fixture small: auth bodies of at most 40 bytes)
  for (auto &m : v)
    if (m.body.mtype() == xdr::CALL) { shrink(m.body.cbody().cred); shrink(m.body.cbody().verf); }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) refobj::die("usage: compare_ref OUT.json");
  writer w{fopen(argv[1], "w")};
  if (!w.f) refobj::die("cannot open output");
  const int N = 8 * kEach;  // candidates per type
  fprintf(w.f, "{\"generator\":\"tests/cpp/compare_ref.cc: the reference's operator<=> (cmp: -1 less, 0 equivalent, "
               "1 greater, 2 unordered) and operator== (eq) on seeded pairs [how, a, b, cmp, eq]; b empty = a again, "
               "@pos=xx = a's bytes with byte pos set to xx\",\n\"types\":{\n");
  {
    vector<testns::numerics> a, o;
    refobj::gen_numerics(N, 0xC0A1, a);
    refobj::gen_numerics(N, 0xC0A2, o);
    auto sp = float_specials<testns::numerics>(
        a[0], [](testns::numerics &t, double v) { t.f2 = v; }, [](testns::numerics &t) { t.i1 ^= 0x40; });
    auto sf = float_specials<testns::numerics>(
        a[0], [](testns::numerics &t, double v) { t.f1 = float(v); }, [](testns::numerics &t) { t.b = !t.b; });
    sp.insert(sp.end(), sf.begin(), sf.end());
    emit(w, "numerics", true, a, o, 0xA171, sp);
  }
  {
    vector<rec128> a, o;
    refobj::gen_rec128(N, 0xC0B1, 0, a);
    refobj::gen_rec128(N, 0xC0B2, 0, o);
    rec128 base = a[0];
    double *dd = &base.d0;
    for (int k = 0; k < 6; ++k) dd[k] = 0.25 * k;  // (random bit patterns may hold a NaN of their own)
    auto sp = float_specials<rec128>(
        base, [](rec128 &t, double v) { t.d3 = v; }, [](rec128 &t) { t.u5 += 1; });
    emit(w, "rec128", true, a, o, 0xA172, sp);
  }
  {
    vector<recvar> a, o;
    refobj::gen_recvar(N, 0xC0C1, a);
    refobj::gen_recvar(N, 0xC0C2, o);
    for (auto *v : {&a, &o})  // (keeps the fixture small: blobs of at most 64 bytes; the GPU tests take 256)
      for (auto &x : *v) x.blob.resize(x.blob.size() % 65);
    auto sp = float_specials<recvar>(
        a[0], [](recvar &t, double v) { t.score = v; }, [](recvar &t) { t.name += "z"; });
    emit(w, "recvar", true, a, o, 0xA173, sp);
  }
  {
    vector<xdr::rpc_msg> a, o;
    refobj::gen_rpc(N, 0xC0D1, a);
    refobj::gen_rpc(N, 0xC0D2, o);
    shrink(a);
    shrink(o);
    emit(w, "rpc_msg", false, a, o, 0xA174, {});
  }
  {
    auto a = many<uunion>(r_uunion, 0xC0E1, N), o = many<uunion>(r_uunion, 0xC0E2, N);
    uunion base(3);
    auto sp = float_specials<uunion>(
        base, [](uunion &t, double v) { t.three() = v; }, [](uunion &t) { t.d(2); t.two() = 7; });
    emit(w, "uunion", true, a, o, 0xA175, sp);
  }
  {
    auto a = many<uptr>(r_uptr, 0xC0F1, N), o = many<uptr>(r_uptr, 0xC0F2, N);
    emit(w, "uptr", false, a, o, 0xA176, {});
  }
  {
    auto a = many<testns::ContainsEnum>(r_contains, 0xC101, N), o = many<testns::ContainsEnum>(r_contains, 0xC102, N);
    vector<pair_t<testns::ContainsEnum>> sp;  // the reference's tests/compare.cc:32-45
    testns::ContainsEnum ce1(REDDER);
    ce1.num() = testns::ContainsEnum::ONE;
    testns::ContainsEnum ce2 = ce1;
    sp.push_back({ce1, ce2, "", "special"});
    ce2.num() = testns::ContainsEnum::TWO;
    sp.push_back({ce1, ce2, "", "special"});
    sp.push_back({ce2, ce1, "", "special"});
    ce1.c(RED);
    ce1.foo() = "hello world";
    sp.push_back({ce1, ce2, "", "special"});
    sp.push_back({ce2, ce1, "", "special"});
    emit(w, "ContainsEnum", false, a, o, 0xA177, sp);
  }
  {
    auto a = many<testns::containertest>(xdrtest_gen::r_containertest, 0xC111, N);
    auto o = many<testns::containertest>(xdrtest_gen::r_containertest, 0xC112, N);
    testns::containertest base;
    base.uvec = {u_4_12(4), u_4_12(12), u_4_12(4)};
    base.uvec[1].f12().i = 3;
    base.sarr[0] = "hello";
    auto sp = float_specials<testns::containertest>(
        base, [](testns::containertest &t, double v) { t.uvec[1].f12().d = v; },
        [](testns::containertest &t) { t.uvec[0].f4().i = -1; });
    // a vector of unions differing in discriminant only
    testns::containertest d1 = base, d2 = base;
    d1.uvec[2] = u_4_12(4);
    d2.uvec[2] = u_4_12(12);
    sp.push_back({d1, d2, "", "special"});
    emit(w, "containertest", true, a, o, 0xA178, sp);
  }
  {
    auto a = many<testns::hasbytes>(xdrtest_gen::r_hasbytes, 0xC121, N);
    auto o = many<testns::hasbytes>(xdrtest_gen::r_hasbytes, 0xC122, N);
    emit(w, "hasbytes", false, a, o, 0xA179, {});
  }
  {
    auto gen = [](rng &g) { return xdrtest_gen::r_recursive(g, 1 + int(g.below(2))); };
    auto a = many<test_recursive>(gen, 0xC131, N), o = many<test_recursive>(gen, 0xC132, N);
    emit(w, "test_recursive", false, a, o, 0xA17A, {});
  }
  {
    vector<xdr::rp__list> a, o;
    refobj::gen_rp_list(N, 0xC141, a);
    refobj::gen_rp_list(N, 0xC142, o);
    emit(w, "rp__list", false, a, o, 0xA17B, {});
  }
  fprintf(w.f, "\n}}\n");
  fclose(w.f);
  return 0;
}
