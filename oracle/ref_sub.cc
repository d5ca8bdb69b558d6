// ORACLE / TEST INFRASTRUCTURE ONLY — never shipped, never measured.
//
// Golden vectors for the element-subroutine layouts of oracle/x/subzoo.x
// (lists, chains that do not end their record, a tail container in a union
// arm, chains through an xvector, trees, nine nested container levels, wide
// elements, two types that contain each other), made by the REAL reference
// marshaler (xdrpp/marshal.cc compiled in place) over GENUINE xdrc output:
// subzoo.hh as the reference's own back end (xdrc/gen_hh.cc) emits it
// (oracle/Makefile, oracle/xdrc_driver.cc).
//
//   ref_sub <out.json>
//
// For every type: sizeof, alignof and the offsetof of every top-level field,
// then 16 records.  A record is described by its shape and a seed, not dumped:
//   "counts": what every pointer (0 / 1), xvector (its size) and union (its
//             discriminant) met in wire order takes, run-length coded
//             [[value, times], ...];
//   "seed":   the splitmix64 state the other fields are drawn from, in wire
//             order: a bool is g() & 1, an int or hyper g() truncated, an enum
//             its (g() % n)-th tag in declaration order, opaque[n] n times
//             uint8(g()), a string or opaque<B> the byte ramp start + j * step
//             (mod 256) of length g() % (B + 1), start g() & 255, step
//             (g() & 255) | 1, drawn in that order.
// Node counts of the list and chain records: kNodes below (a record that is
// itself the list's first node has no null head: it takes 1 node there).
// Emitted per record: xdr_to_opaque (hex up to 512 bytes; longer: its size,
// sha256 and first 32 bytes), the smallest level check_xdr_depth accepts, the
// smallest marshaling_stack_limit under which xdr_to_opaque / xdr_from_opaque
// succeed (by bisection), whether what xdr_from_opaque makes of it marshals to
// the same bytes, and
// the exception class of xdr_from_opaque on damaged copies of the record.
// The damage is placed by the record's own fields, at the middle one of its
// kind (so in a list it falls in a middle node): a bool word of 2, an enum
// word of 3, a non-zero pad byte after an opaque[n] and after a payload, a
// pointer count of 2, a length within its bound that runs one byte past the
// record (the last payload that allows it), one trailing word, the record cut
// by one word.  The reference reads any non-zero bool word as true, so the
// "bool" copies are accepted ("none") and held as that; any other damaged
// copy the reference accepts ends the generator.
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include <xdrpp/depth_checker.h>
#include <xdrpp/marshal.h>

#include "ref_util.hh"
#include "subzoo.hh"

namespace subzoo {
template <typename T> inline void xdr_validate_enum(T);  // tests/validate.cc:18-20
}

using namespace subzoo;
using namespace ref_util;
using std::string;
using std::vector;

namespace {

constexpr int kRecords = 16;
// kChainT = 32, the list decode's 64-node batch, kChainChunk = 64 (sub_kernels.h)
constexpr uint32_t kNodes[kRecords] = {0, 1, 2, 31, 32, 33, 34, 63, 64, 65, 66, 100, 129, 5, 96, 199};
using counts_t = vector<uint32_t>;

// An archive that builds what it visits (xdr_traits<T>::load walks a struct's
// fields through it).
struct filler {
  rng &g;
  const counts_t &counts;
  size_t ci = 0;
  uint32_t take() {
    if (ci >= counts.size()) { fprintf(stderr, "counts ran out\n"); exit(1); }
    return counts[ci++];
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_numeric>::type operator()(T &t) {
    using U = typename xdr::xdr_traits<T>::uint_type;
    t = xdr::xdr_traits<T>::from_uint(U(g()));
  }
  // (bool is an enum to the reference's traits)
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_enum>::type operator()(T &t) {
    if constexpr (std::is_same<T, bool>::value) {
      t = bool(g() & 1);
    } else {
      const auto &v = xdr::xdr_traits<T>::enum_values();
      t = T(v[g() % v.size()]);
    }
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_bytes>::type operator()(T &t) {
    if constexpr (xdr::xdr_traits<T>::variable_nelem) {
      t.resize(size_t(g() % (uint64_t(t.max_size()) + 1)));
      const unsigned start = unsigned(g() & 0xff), step = unsigned(g() & 0xff) | 1u;
      for (size_t j = 0; j < t.size(); ++j) t[j] = uint8_t(start + j * step);
    } else {
      for (auto &b : t) b = uint8_t(g());
    }
  }
  template <typename T> void operator()(xdr::pointer<T> &p) {
    if (take()) (*this)(p.activate()); else p.reset();
  }
  void operator()(utail &u) {
    u.k(int32_t(take()));
    if (u.k() == 1) (*this)(u.next());
    if (u.k() == 2) (*this)(u.alt());
  }
  template <typename T>
  typename std::enable_if<xdr::xdr_traits<T>::is_class && !xdr::xdr_traits<T>::is_union>::type operator()(T &t) {
    xdr::xdr_traits<T>::load(*this, t);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_container>::type operator()(T &t) {
    if constexpr (xdr::xdr_traits<T>::variable_nelem) t.resize(take());
    for (auto &e : t) xdr::archive(*this, e);
  }
};

// One place on the wire that damage can go.
struct site {
  char kind;  // b bool, e enum, f opaque[n] with a pad, v payload (its length word), p pointer count
  size_t pos;
  uint32_t len, bound;
};

// An archive that notes where the fields sit on the wire.
struct scout {
  size_t pos = 0;
  vector<site> sites;
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_numeric>::type operator()(const T &) {
    pos += sizeof(typename xdr::xdr_traits<T>::uint_type);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_enum>::type operator()(const T &) {
    sites.push_back({std::is_same<T, bool>::value ? 'b' : 'e', pos, 0, 0});
    pos += 4;
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_bytes>::type operator()(const T &t) {
    if constexpr (xdr::xdr_traits<T>::variable_nelem) {
      sites.push_back({'v', pos, uint32_t(t.size()), uint32_t(t.max_size())});
      pos += 4;
    } else if (t.size() % 4) {
      sites.push_back({'f', pos, uint32_t(t.size()), 0});
    }
    pos += (t.size() + 3) & ~size_t(3);
  }
  template <typename T> void operator()(const xdr::pointer<T> &p) {
    sites.push_back({'p', pos, 0, 0});
    pos += 4;
    if (p) (*this)(*p);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_class>::type operator()(const T &t) {
    xdr::xdr_traits<T>::save(*this, t);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_container>::type operator()(const T &t) {
    if (xdr::xdr_traits<T>::variable_nelem) pos += 4;
    for (const auto &e : t) xdr::archive(*this, e);
  }
};

}  // namespace

namespace xdr {
template <> struct archive_adapter<scout> {
  template <typename T> static void apply(scout &s, const T &t, const char *) { s(t); }
};
}  // namespace xdr

namespace {

struct edit {
  string kind;
  size_t offset;
  vector<uint8_t> w;
  int resize;
};

vector<uint8_t> be32(uint32_t v) { return {uint8_t(v >> 24), uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)}; }

vector<edit> damages(const vector<site> &sites, size_t size) {
  vector<edit> out;
  auto mid = [&](const std::function<bool(const site &)> &ok) -> const site * {
    vector<const site *> c;
    for (const site &s : sites)
      if (ok(s)) c.push_back(&s);
    return c.empty() ? nullptr : c[c.size() / 2];
  };
  if (const site *s = mid([](const site &y) { return y.kind == 'b'; })) out.push_back({"bool", s->pos, be32(2), 0});
  if (const site *s = mid([](const site &y) { return y.kind == 'e'; })) out.push_back({"enum", s->pos, be32(3), 0});
  if (const site *s = mid([](const site &y) { return y.kind == 'f'; }))
    out.push_back({"pad_fixed", s->pos + s->len, {0x01}, 0});
  if (const site *s = mid([](const site &y) { return y.kind == 'v' && y.len % 4; }))
    out.push_back({"pad", s->pos + 4 + s->len, {0x5a}, 0});
  if (const site *s = mid([](const site &y) { return y.kind == 'p'; })) out.push_back({"count", s->pos, be32(2), 0});
  for (size_t k = sites.size(); k-- > 0;) {
    const site &y = sites[k];
    const size_t rest = size - y.pos - 4;
    if (y.kind == 'v' && rest + 1 <= y.bound) {
      out.push_back({"past", y.pos, be32(uint32_t(rest + 1)), 0});
      break;
    }
  }
  out.push_back({"trailing", 0, {}, 4});
  if (size >= 4) out.push_back({"truncated", 0, {}, -4});
  return out;
}

template <typename T> string exception_of(const vector<uint8_t> &wire) {
  T back;
  try {
    xdr::xdr_from_opaque(wire, back);
  }
#define CATCH(C) catch (const xdr::C &) { return #C; }
  CATCH(xdr_should_be_zero)
  CATCH(xdr_invariant_failed)
  CATCH(xdr_bad_discriminant)
  CATCH(xdr_bad_message_size)
  CATCH(xdr_stack_overflow)
  CATCH(xdr_overflow)
#undef CATCH
  catch (const std::exception &) { return "other"; }
  return "none";
}

// smallest L in [0, hi] with ok(L) (ok monotone, ok(hi) true)
template <typename F> uint32_t bisect(uint32_t hi, F ok) {
  uint32_t lo = 0;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (ok(m)) hi = m; else lo = m + 1;
  }
  return hi;
}
template <typename F> bool no_overflow(uint32_t L, F f) {
  xdr::marshaling_stack_limit = L;
  bool ok = true;
  try { f(); } catch (const xdr::xdr_stack_overflow &) { ok = false; }
  xdr::marshaling_stack_limit = 0xffffffff;
  return ok;
}

string rle(const counts_t &c) {
  string s = "[";
  for (size_t i = 0; i < c.size();) {
    size_t j = i;
    while (j < c.size() && c[j] == c[i]) ++j;
    s += string(i ? ", " : "") + "[" + std::to_string(c[i]) + ", " + std::to_string(j - i) + "]";
    i = j;
  }
  return s + "]";
}

template <typename T>
string emit(const char *name, const string &offs_json, uint64_t seed, const std::function<counts_t(int)> &shape) {
  std::ostringstream o;
  o << q(name) << ": {\"sizeof\": " << sizeof(T) << ", \"alignof\": " << alignof(T) << ", \"offsetof\": {"
    << offs_json << "},\n  \"records\": [";
  for (int r = 0; r < kRecords; ++r) {
    const counts_t counts = shape(r);
    const uint64_t rseed = seed * 1000003ull + uint64_t(r);
    rng g{rseed};
    T v;
    filler f{g, counts};
    f(v);
    if (f.ci != counts.size()) { fprintf(stderr, "%s: record %d leaves counts over\n", name, r); exit(1); }
    scout s;
    s(v);
    const auto m = xdr::xdr_to_opaque(v);
    if (m.size() != s.pos) {
      fprintf(stderr, "%s: record %d is %zu bytes, walked %zu\n", name, r, size_t(m.size()), s.pos);
      exit(1);
    }
    const vector<uint8_t> wire(m.begin(), m.end());
    const uint32_t hi = 4096;
    const uint32_t depth = bisect(hi, [&](uint32_t L) { return xdr::check_xdr_depth(v, L); });
    const uint32_t put = bisect(hi, [&](uint32_t L) { return no_overflow(L, [&] { (void)xdr::xdr_to_opaque(v); }); });
    const uint32_t get = bisect(hi, [&](uint32_t L) {
      return no_overflow(L, [&] { T t; xdr::xdr_from_opaque(wire, t); });
    });
    T back;
    xdr::xdr_from_opaque(wire, back);
    const auto again = xdr::xdr_to_opaque(back);  // (the generated types of a namespace have no operator==)
    const bool same = again.size() == wire.size() && !memcmp(again.data(), wire.data(), wire.size());
    o << (r ? ",\n    " : "\n    ") << "{\"seed\": " << rseed << ", \"counts\": " << rle(counts) << ", \"size\": "
      << wire.size() << ", ";
    if (wire.size() <= 512)
      o << "\"xdr\": " << q(hex(wire.data(), wire.size()));
    else
      o << "\"xdr_sha256\": " << q(sha256(wire.data(), wire.size())) << ", \"xdr_head\": " << q(hex(wire.data(), 32));
    o << ", \"depth\": " << depth << ", \"put_limit\": " << put << ", \"get_limit\": " << get
      << ", \"round_trip\": " << (same ? "true" : "false") << ",\n     \"damaged\": [";
    const vector<edit> dmg = damages(s.sites, wire.size());
    for (size_t k = 0; k < dmg.size(); ++k) {
      const edit &d = dmg[k];
      vector<uint8_t> bad = wire;
      std::copy(d.w.begin(), d.w.end(), bad.begin() + d.offset);
      bad.resize(bad.size() + d.resize, 0);
      const string exc = exception_of<T>(bad);
      if (exc == "none" && d.kind != "bool") {
        fprintf(stderr, "%s: record %d: the reference accepts damage %s\n", name, r, d.kind.c_str());
        exit(1);
      }
      o << (k ? ", " : "") << "[" << q(d.kind) << ", " << d.offset << ", " << q(hex(d.w.data(), d.w.size())) << ", "
        << d.resize << ", " << q(exc) << "]";
    }
    o << "]}";
  }
  o << "]}";
  return o.str();
}

#define OFF(T, f) (string("\"" #f "\": ") + std::to_string(offsetof(T, f)))
string join(std::initializer_list<string> l) {
  string s;
  for (const string &x : l) s += (s.empty() ? "" : ", ") + x;
  return s;
}

void add(counts_t &c, uint32_t v, uint32_t n) { c.insert(c.end(), n, v); }
// a list of k nodes behind a pointer (k = 0: null)
void chain(counts_t &c, uint32_t k) { add(c, 1, k); c.push_back(0); }
// a record that is the first of k nodes (k >= 1)
counts_t root_chain(uint32_t k) {
  counts_t c;
  chain(c, std::max(k, 1u) - 1);
  return c;
}

// tree shapes, in wire order: l's count, the left subtree, r's count, the right subtree
void balanced(counts_t &c, int depth) {  // a full tree of `depth` levels
  for (int side = 0; side < 2; ++side) {
    c.push_back(depth > 1);
    if (depth > 1) balanced(c, depth - 1);
  }
}
void spine(counts_t &c, uint32_t nodes, bool left, bool leaves) {  // `nodes` down one side (leaves: each with a leaf
  if (left) {                                                      // on the other side)
    c.push_back(nodes > 1);
    if (nodes > 1) spine(c, nodes - 1, left, leaves);
    c.push_back(leaves && nodes > 1);
    if (leaves && nodes > 1) add(c, 0, 2);
  } else {
    c.push_back(leaves && nodes > 1);
    if (leaves && nodes > 1) add(c, 0, 2);
    c.push_back(nodes > 1);
    if (nodes > 1) spine(c, nodes - 1, left, leaves);
  }
}
void zigzag(counts_t &c, uint32_t nodes, bool left) {
  if (left) {
    c.push_back(nodes > 1);
    if (nodes > 1) zigzag(c, nodes - 1, false);
    c.push_back(0);
  } else {
    c.push_back(0);
    c.push_back(nodes > 1);
    if (nodes > 1) zigzag(c, nodes - 1, true);
  }
}
void random_tree(counts_t &c, rng &g, uint32_t &budget) {
  for (int side = 0; side < 2; ++side) {
    const bool kid = budget > 0 && g() % 3 != 0;
    c.push_back(kid);
    if (kid) { --budget; random_tree(c, g, budget); }
  }
}

// `levels` nested vectors, each of 0, 1 or 3 elements; at most two levels of 3 on a path
void nest(counts_t &c, rng &g, int levels, int threes, int mode) {
  if (!levels) return;
  uint32_t n = mode == 0 ? 0 : mode == 1 ? 1 : uint32_t((g() % 3) * 3 / 2);  // 0, 1, 3
  if (mode == 2 && levels > 7) n = std::max(n, 1u);
  if (n == 3 && !threes) n = 1;
  c.push_back(n);
  for (uint32_t i = 0; i < n; ++i) nest(c, g, levels - 1, threes - (n == 3), mode);
}
counts_t nest_record(int levels, int r) {
  counts_t c;
  rng g{uint64_t(0x6e657374 + 131 * r + levels)};
  if (r == 0) nest(c, g, levels, 2, 0);        // empty at the top
  else if (r == 1) nest(c, g, levels, 2, 1);   // one element at every level: full to the bottom
  else if (r == 2) {                           // 3 at the top and at the bottom, 1 between: full to the bottom
    c.push_back(3);
    for (int e = 0; e < 3; ++e) { add(c, 1, levels - 2); c.push_back(3); }
  } else nest(c, g, levels, 2, 2);
  return c;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ref_sub <out.json>\n");
    return 2;
  }
  vector<string> out;
  uint64_t seed = 0x7375627a6f6f21ull;
  const auto list = [](int r) { return root_chain(kNodes[r]); };
#define ZOO(T, shape, ...) out.push_back(emit<T>(#T, join({__VA_ARGS__}), ++seed, shape))
  ZOO(flatlist, list, OFF(flatlist, b), OFF(flatlist, e), OFF(flatlist, h), OFF(flatlist, fx), OFF(flatlist, o),
      OFF(flatlist, s), OFF(flatlist, next));
  ZOO(widelist, list, OFF(widelist, v), OFF(widelist, a), OFF(widelist, tail), OFF(widelist, b), OFF(widelist, next));
  ZOO(oddlist, list, OFF(oddlist, a), OFF(oddlist, s), OFF(oddlist, next));
  ZOO(holder, [](int r) { counts_t c; chain(c, kNodes[r]); return c; }, OFF(holder, a), OFF(holder, head),
      OFF(holder, after), OFF(holder, z));
  // a then b: the node counts and the counts five records on, so both chains pass 32 nodes in some records
  ZOO(twolists, [](int r) { counts_t c; chain(c, kNodes[r]); chain(c, kNodes[(r + 5) % kRecords]); return c; },
      OFF(twolists, a), OFF(twolists, b));
  // r % 4 lists (records 12 to 15: 1 to 4), of the node counts from r on, at most 70 nodes each
  ZOO(listvec, [](int r) {
        counts_t c;
        const uint32_t m = r < 12 ? r % 4 : r - 11;
        c.push_back(m);
        for (uint32_t j = 0; j < m; ++j) {
          const counts_t e = root_chain(std::min(kNodes[(r + 7 * j) % kRecords], 70u));
          c.insert(c.end(), e.begin(), e.end());
        }
        return c;
      }, OFF(listvec, heads));
  // the last node's union: void, alt, or a null next, by the record
  ZOO(unode, [](int r) {
        counts_t c;
        add(c, 1, 2 * (std::max(kNodes[r], 1u) - 1));
        if (r % 3 == 0) c.push_back(0);
        else if (r % 3 == 1) c.push_back(2);
        else { c.push_back(1); c.push_back(0); }
        return c;
      }, OFF(unode, s), OFF(unode, t));
  // records 13 and 14: 60 nodes with a 3-element kids at node 5 and at node 40 (its first two kids are leaves)
  ZOO(vchain, [](int r) {
        if (r != 13 && r != 14) return root_chain(kNodes[r]);
        const uint32_t at = r == 13 ? 5 : 40;
        counts_t c;
        add(c, 1, at);
        c.push_back(3);
        add(c, 0, 2);
        add(c, 1, 60 - at - 2);
        c.push_back(0);
        return c;
      }, OFF(vchain, s), OFF(vchain, kids));
  ZOO(tree, [](int r) {
        counts_t c;
        rng g{uint64_t(0x74726565 + r)};
        uint32_t budget = 50;
        if (r < 6) balanced(c, r + 1);                 // balanced, 1 to 6 levels
        else if (r == 6) spine(c, 12, true, false);    // left spines: past the 8 register frames,
        else if (r == 7) spine(c, 9, true, false);     // one past them,
        else if (r == 8) spine(c, 8, true, false);     // and within them
        else if (r == 9) spine(c, 70, false, false);   // right spines: replacements past kChainT
        else if (r == 10) spine(c, 33, false, false);
        else if (r == 11) spine(c, 34, false, false);
        else if (r == 12) spine(c, 12, true, true);    // a left spine whose nodes have right leaves
        else if (r == 13) spine(c, 40, false, true);   // a right spine whose nodes have left leaves
        else if (r == 14) zigzag(c, 40, true);
        else random_tree(c, g, budget);
        return c;
      }, OFF(tree, key), OFF(tree, s), OFF(tree, l), OFF(tree, r));
  ZOO(nest8, [](int r) { return nest_record(8, r); }, OFF(nest8, top));
  ZOO(nest9, [](int r) { return nest_record(9, r); }, OFF(nest9, top));
  const auto vec = [](int r) { return counts_t{kNodes[r]}; };
  ZOO(el64, vec, OFF(el64, v));
  ZOO(el72, vec, OFF(el72, v));
  ZOO(ping, list, OFF(ping, s), OFF(ping, p));
#undef ZOO

  std::ofstream f(argv[1]);
  f << "{\"generator\": \"oracle/ref_sub.cc over genuine xdrc output of oracle/x/subzoo.x\",\n"
    << "\"records\": " << kRecords << ",\n"
    << "\"cxx\": {\"opaque_vec\": [" << sizeof(xdr::opaque_vec<>) << ", " << alignof(xdr::opaque_vec<>)
    << "], \"xstring\": [" << sizeof(xdr::xstring<>) << ", " << alignof(xdr::xstring<>) << "], \"pointer\": ["
    << sizeof(xdr::pointer<int>) << ", " << alignof(xdr::pointer<int>) << "], \"xvector\": ["
    << sizeof(xdr::xvector<int>) << ", " << alignof(xdr::xvector<int>) << "]},\n\"structs\": {\n";
  for (size_t k = 0; k < out.size(); ++k) f << out[k] << (k + 1 < out.size() ? ",\n" : "\n");
  f << "}\n}\n";
  f.close();
  return f ? 0 : 1;
}
