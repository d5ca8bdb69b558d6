// ORACLE / TEST INFRASTRUCTURE ONLY — never shipped, never measured.
//
// Golden vectors for the variable-length layouts of oracle/x/varzoo.x, made
// by the REAL reference marshaler (xdrpp/marshal.cc compiled in place) over
// GENUINE xdrc output: varzoo.hh as the reference's own back end
// (xdrc/gen_hh.cc) emits it (oracle/Makefile, oracle/xdrc_driver.cc).
//
//   ref_var <out.json>
//
// For every struct: sizeof, alignof and the offsetof of every top-level
// field (the C++ layout; a payload field there is a std::vector or
// std::string, whose sizes head the file), then 16 records.  The records are
// not random in their lengths: payload k of record i (k counts the payloads
// in wire order) has the length kCycle[(i + 5 * k) % 16], clipped to its
// bound B, with B - 1 and B the cycle's last two entries (an unbounded field
// takes B = 1000); `four` empties field k exactly where bit k of i is set, so
// its records run through all 16 empty / non-empty combinations; long9k's
// opaque<9000> takes the lengths around the 4 and 8 KiB images; armslots goes
// round its arms and mixed's pointer is set in every other record.  A payload
// is the byte ramp start + j * step (mod 256), written [start, step, length];
// the other fields come from a seeded generator (splitmix64).
// Emitted: the values, each record's wire size, xdr_to_opaque of the records
// back to back (streams over 2 KiB: sha256 and the first 64 bytes), what
// xdr_from_opaque makes of each record ("values" where that is the values
// again), and the reference's verdict on damaged streams -- each record
// unmarshaled from its own bytes, the last one from whatever the stream has
// left: the first record xdr_from_opaque throws on, the exception's class and
// its what().
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

#include <xdrpp/marshal.h>

#include "ref_util.hh"
#include "varzoo.hh"

namespace varzoo {
template <typename T> inline void xdr_validate_enum(T);  // tests/validate.cc:18-20
}

using namespace varzoo;
using namespace ref_util;
using std::string;
using std::vector;

namespace {

constexpr int kRecords = 16;
constexpr uint32_t kUnboundedAs = 1000;  // the bound the length cycle gives an unbounded field
// (B - 1 and B stand in for the last two entries)
constexpr int kCycle[kRecords] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, -1, -2};

uint32_t cycle_len(int i, int k, uint32_t B) {
  B = std::min(B, kUnboundedAs);
  const int c = kCycle[(i + 5 * k) % kRecords];
  if (c < 0) return B - uint32_t(c == -1);
  return std::min(uint32_t(c), B);
}

// (record, payload index, bound) -> length, or -1 for the cycle's
using len_rule = std::function<long(int, int, uint32_t)>;

// An archive that fills what it visits (xdr_traits<T>::load walks a struct's
// fields through it).
struct filler {
  rng &g;
  int rec;
  const len_rule &rule;
  int k = 0;  // payloads seen in this record
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_numeric>::type operator()(T &t) {
    using U = typename xdr::xdr_traits<T>::uint_type;
    t = xdr::xdr_traits<T>::from_uint(U(g()));
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_enum>::type operator()(T &t) {
    const auto &v = xdr::xdr_traits<T>::enum_values();
    t = T(v[g() % v.size()]);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_bytes>::type operator()(T &t) {
    if constexpr (xdr::xdr_traits<T>::variable_nelem) {
      const uint32_t B = uint32_t(t.max_size());
      long n = rule ? rule(rec, k, B) : -1;
      if (n < 0) n = cycle_len(rec, k, B);
      ++k;
      t.resize(size_t(n));
      const unsigned start = unsigned(g() & 0xff), step = unsigned(g() & 0xff) | 1u;
      for (size_t j = 0; j < t.size(); ++j) t[j] = uint8_t(start + j * step);
    } else {
      for (auto &b : t) b = uint8_t(g());
    }
  }
  template <typename T> void operator()(xdr::pointer<T> &p) {
    if (rec & 1) (*this)(p.activate()); else p.reset();
  }
  void operator()(armu &u) {
    u.which(rec % 3);
    if (u.which() == 1) (*this)(u.a());
    if (u.which() == 2) (*this)(u.t());
  }
  template <typename T>
  typename std::enable_if<xdr::xdr_traits<T>::is_class && !xdr::xdr_traits<T>::is_union>::type operator()(T &t) {
    xdr::xdr_traits<T>::load(*this, t);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_container>::type operator()(T &t) {
    for (auto &e : t) xdr::archive(*this, e);
  }
};

// One payload on the wire: where its length word is, its length, its bound.
struct payload {
  size_t lenpos;
  uint32_t len, bound;
};

// An archive that writes the values it visits as JSON and notes where the
// payloads sit on the wire (xdr_traits<T>::save walks the fields through it,
// with their names: archive_adapter below).
struct scribe {
  string json;
  size_t pos = 0;
  vector<payload> pays;
  vector<int> count{0};  // members written at each open level
  vector<char> kind{'v'};  // 'o' object (named members), 'l' list or union

  void member(const char *name) {
    if (count.back()++) json += ", ";
    if (kind.back() == 'o') json += q(name ? name : "?") + ": ";
  }
  void open(char k, const char *bracket) {
    json += bracket;
    count.push_back(0);
    kind.push_back(k);
  }
  void close(const char *bracket) {
    json += bracket;
    count.pop_back();
    kind.pop_back();
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_numeric>::type operator()(const T &t) {
    if (std::is_same<T, bool>::value) json += t ? "true" : "false";
    else if (std::is_floating_point<T>::value) abort();  // (no float fields here: they have no exact JSON)
    else json += std::to_string(t);
    pos += sizeof(typename xdr::xdr_traits<T>::uint_type);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_enum>::type operator()(const T &t) {
    json += std::to_string(int32_t(t));
    pos += 4;
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_bytes>::type operator()(const T &t) {
    if constexpr (xdr::xdr_traits<T>::variable_nelem) {
      const unsigned start = t.size() ? uint8_t(t[0]) : 0;
      const unsigned step = t.size() > 1 ? uint8_t(uint8_t(t[1]) - uint8_t(t[0])) : 1;
      for (size_t j = 0; j < t.size(); ++j)
        if (uint8_t(t[j]) != uint8_t(start + j * step)) abort();  // (payloads are ramps)
      json += "[" + std::to_string(start) + ", " + std::to_string(step) + ", " + std::to_string(t.size()) + "]";
      pays.push_back({pos, uint32_t(t.size()), uint32_t(t.max_size())});
      pos += 4;
    } else {
      json += q(hex(t.data(), t.size()));
    }
    pos += (t.size() + 3) & ~size_t(3);
  }
  template <typename T> void operator()(const xdr::pointer<T> &p) {
    pos += 4;
    if (p) (*this)(*p); else json += "null";
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_class>::type operator()(const T &t) {
    const bool u = xdr::xdr_traits<T>::is_union;  // a union: [discriminant, arm or null]
    open(u ? 'l' : 'o', u ? "[" : "{");
    xdr::xdr_traits<T>::save(*this, t);
    if (u && count.back() == 1) json += ", null";
    close(u ? "]" : "}");
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_container>::type operator()(const T &t) {
    open('l', "[");
    for (const auto &e : t) xdr::archive(*this, e);
    close("]");
  }
};

}  // namespace

namespace xdr {
template <> struct archive_adapter<scribe> {
  template <typename T> static void apply(scribe &s, const T &t, const char *name) {
    s.member(name);
    s(t);
  }
};
}  // namespace xdr

namespace {

struct edit {
  string kind;
  int record;
  size_t offset;      // in the record's wire bytes
  vector<uint8_t> w;  // written there
  int resize;         // bytes added to (cut from) the stream's end
};

// The first record of `wire` the reference throws on, each unmarshaled from
// its own bytes (offs), the last one from what is left of the stream.
template <typename T> string verdict(const vector<uint8_t> &wire, const vector<size_t> &offs) {
  for (int r = 0; r < kRecords; ++r) {
    const size_t end = r + 1 < kRecords ? offs[r + 1] : wire.size();
    const vector<uint8_t> one(wire.begin() + offs[r], wire.begin() + end);
    T back;
    string exc;
    try {
      xdr::xdr_from_opaque(one, back);
      continue;
    }
#define CATCH(C) catch (const xdr::C &e) { exc = string("\"exception\": \"" #C "\", \"what\": ") + q(e.what()); }
    CATCH(xdr_should_be_zero)
    CATCH(xdr_invariant_failed)
    CATCH(xdr_bad_discriminant)
    CATCH(xdr_bad_message_size)
    CATCH(xdr_stack_overflow)
    CATCH(xdr_overflow)
#undef CATCH
    catch (const std::exception &e) {
      exc = string("\"exception\": \"other\", \"what\": ") + q(e.what());
    }
    return "\"record\": " + std::to_string(r) + ", " + exc;
  }
  return "\"record\": null, \"exception\": \"none\", \"what\": \"\"";
}

vector<uint8_t> be32(uint32_t v) { return {uint8_t(v >> 24), uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)}; }

// The damage every struct gets, placed by its records' own payloads.
vector<edit> damages(const vector<vector<payload>> &pays, const vector<size_t> &sizes) {
  vector<edit> out;
  auto first = [&](int from, const std::function<bool(int, const payload &, bool)> &ok, const payload **hit) {
    for (int d = 0; d < kRecords; ++d) {
      const int r = (from + d) % kRecords;
      for (size_t k = pays[r].size(); k-- > 0;)
        if (ok(r, pays[r][k], k + 1 == pays[r].size())) { *hit = &pays[r][k]; return r; }
    }
    return -1;
  };
  const payload *p = nullptr;
  // a nonzero pad byte after a payload
  int r = first(5, [](int, const payload &y, bool) { return y.len % 4 != 0; }, &p);
  if (r >= 0) out.push_back({"pad", r, p->lenpos + 4 + p->len, {0x5a}, 0});
  // a length one past the bound, its bytes inside the record where a record has them
  auto rest = [&](int rr, const payload &y) { return sizes[rr] - y.lenpos - 4; };
  r = first(9, [&](int rr, const payload &y, bool) { return y.bound != xdr::XDR_MAX_LEN && rest(rr, y) >= y.bound + 1; }, &p);
  if (r < 0) r = first(9, [&](int, const payload &y, bool) { return y.bound != xdr::XDR_MAX_LEN && y.len == y.bound; }, &p);
  if (r >= 0) out.push_back({"bound", r, p->lenpos, be32(p->bound + 1), 0});
  // a length within the bound that runs past the record
  r = first(12, [&](int rr, const payload &y, bool) { return rest(rr, y) + 1 <= y.bound; }, &p);
  if (r >= 0) out.push_back({"past", r, p->lenpos, be32(uint32_t(rest(r, *p) + 1)), 0});
  out.push_back({"truncated", kRecords - 1, 0, {}, -4});
  out.push_back({"trailing", kRecords - 1, 0, {}, 4});
  return out;
}

template <typename T>
string emit(const char *name, const string &offs_json, uint64_t seed, const len_rule &rule,
            const vector<edit> &extra) {
  vector<T> v(kRecords);
  rng g{seed};
  vector<uint8_t> wire;
  vector<size_t> offs, sizes;
  vector<vector<payload>> pays;
  string values, decoded;
  bool same = true;
  for (int r = 0; r < kRecords; ++r) {
    filler f{g, r, rule};
    f(v[r]);
    scribe s;
    s(v[r]);
    const auto m = xdr::xdr_to_opaque(v[r]);
    if (m.size() != s.pos) {
      fprintf(stderr, "%s: record %d is %zu bytes, walked %zu\n", name, r, size_t(m.size()), s.pos);
      exit(1);
    }
    offs.push_back(wire.size());
    sizes.push_back(m.size());
    pays.push_back(s.pays);
    wire.insert(wire.end(), m.begin(), m.end());
    T back;
    xdr::xdr_from_opaque(m, back);
    scribe d;
    d(back);
    same = same && d.json == s.json;
    values += string(r ? ",\n    " : "\n    ") + s.json;
    decoded += string(r ? ",\n    " : "\n    ") + d.json;
  }
  std::ostringstream o;
  o << q(name) << ": {\"sizeof\": " << sizeof(T) << ", \"alignof\": " << alignof(T) << ",\n  \"offsetof\": {"
    << offs_json << "},\n  \"values\": [" << values << "],\n  \"sizes\": [";
  for (int r = 0; r < kRecords; ++r) o << (r ? ", " : "") << sizes[r];
  o << "],\n";
  if (wire.size() <= 2048)
    o << "  \"xdr\": " << q(hex(wire.data(), wire.size())) << ",\n";
  else
    o << "  \"xdr_sha256\": " << q(sha256(wire.data(), wire.size())) << ",\n"
      << "  \"xdr_head\": " << q(hex(wire.data(), 64)) << ",\n";
  if (same) o << "  \"decoded\": \"values\",\n";
  else o << "  \"decoded\": [" << decoded << "],\n";
  vector<edit> dmg = damages(pays, sizes);
  dmg.insert(dmg.end(), extra.begin(), extra.end());
  o << "  \"damaged\": [";
  for (size_t k = 0; k < dmg.size(); ++k) {
    const edit &d = dmg[k];
    vector<uint8_t> bad = wire;
    std::copy(d.w.begin(), d.w.end(), bad.begin() + offs[d.record] + d.offset);
    bad.resize(bad.size() + d.resize, 0);
    o << (k ? ",\n    " : "\n    ") << "{\"kind\": " << q(d.kind) << ", \"at_record\": " << d.record
      << ", \"offset\": " << d.offset << ", \"write\": " << q(hex(d.w.data(), d.w.size()))
      << ", \"resize\": " << d.resize << ", " << verdict<T>(bad, offs) << "}";
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

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ref_var <out.json>\n");
    return 2;
  }
  vector<string> out;
  uint64_t seed = 0x7661727a6f6f2121ull;
  const len_rule cycle;
#define ZOO(T, rule, extra, ...) out.push_back(emit<T>(#T, join({__VA_ARGS__}), ++seed, rule, extra))
  ZOO(one, cycle, {}, OFF(one, o));
  ZOO(three, cycle, {}, OFF(three, a), OFF(three, b), OFF(three, i), OFF(three, c));
  // field k empty exactly where bit k of the record's number is set
  const len_rule combos = [](int i, int k, uint32_t B) -> long {
    if (i >> k & 1) return 0;
    const uint32_t n = cycle_len(i, k, B);
    return n ? n : B;
  };
  ZOO(four, combos, {}, OFF(four, a), OFF(four, h), OFF(four, b), OFF(four, c), OFF(four, d));
  ZOO(five, cycle, {}, OFF(five, a), OFF(five, b), OFF(five, i), OFF(five, c), OFF(five, d), OFF(five, e));
  ZOO(str8, cycle, {}, OFF(str8, s0), OFF(str8, s1), OFF(str8, s2), OFF(str8, s3), OFF(str8, s4), OFF(str8, s5),
      OFF(str8, s6), OFF(str8, s7));
  ZOO(str9, cycle, {}, OFF(str9, s0), OFF(str9, s1), OFF(str9, s2), OFF(str9, s3), OFF(str9, s4), OFF(str9, s5),
      OFF(str9, s6), OFF(str9, s7), OFF(str9, s8));
  ZOO(w22, cycle, {}, OFF(w22, v), OFF(w22, o));
  ZOO(w24, cycle, {}, OFF(w24, v), OFF(w24, o));
  ZOO(wide136, cycle, {}, OFF(wide136, v), OFF(wide136, o));
  // the opaque<9000>: lengths around the 4 and 8 KiB images in the even records
  const len_rule images = [](int i, int k, uint32_t) -> long {
    static const long L[8] = {0, 4091, 4092, 4093, 8191, 8192, 8999, 9000};
    return k == 0 && i % 2 == 0 ? L[i / 2] : -1;
  };
  ZOO(long9k, images, {}, OFF(long9k, i), OFF(long9k, o), OFF(long9k, s));
  ZOO(unbounded, cycle, {}, OFF(unbounded, i), OFF(unbounded, o), OFF(unbounded, s));
  ZOO(tiny, cycle, {}, OFF(tiny, o));
  ZOO(mixed, cycle, (vector<edit>{{"pad_fixed", 6, 4 + 5, {0x01}, 0}}), OFF(mixed, b0), OFF(mixed, fx), OFF(mixed, o),
      OFF(mixed, p), OFF(mixed, b1));
  ZOO(armslots, cycle, (vector<edit>{{"discriminant", 7, 0, be32(3), 0}, {"discriminant", 2, 0, be32(0xffffffffu), 0}}),
      OFF(armslots, u), OFF(armslots, tail));
  ZOO(venum, cycle, (vector<edit>{{"enum", 4, 0, be32(3), 0}, {"enum", 11, 0, be32(0), 0}}), OFF(venum, e),
      OFF(venum, s));
#undef ZOO

  std::ofstream f(argv[1]);
  f << "{\"generator\": \"oracle/ref_var.cc over genuine xdrc output of oracle/x/varzoo.x\",\n"
    << "\"records\": " << kRecords << ",\n"
    << "\"cxx\": {\"opaque_vec\": [" << sizeof(xdr::opaque_vec<>) << ", " << alignof(xdr::opaque_vec<>)
    << "], \"xstring\": [" << sizeof(xdr::xstring<>) << ", " << alignof(xdr::xstring<>) << "], \"pointer\": ["
    << sizeof(xdr::pointer<int>) << ", " << alignof(xdr::pointer<int>) << "]},\n\"structs\": {\n";
  for (size_t k = 0; k < out.size(); ++k) f << out[k] << (k + 1 < out.size() ? ",\n" : "\n");
  f << "}\n}\n";
  f.close();
  return f ? 0 : 1;
}
