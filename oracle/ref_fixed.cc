// ORACLE / TEST INFRASTRUCTURE ONLY — never shipped, never measured.
//
// Golden vectors for the awkward fixed-size layouts of oracle/x/fixedzoo.x,
// made by the REAL reference marshaler (xdrpp/marshal.cc compiled in place)
// over GENUINE xdrc output: fixedzoo.hh as the reference's own back end
// (xdrc/gen_hh.cc) emits it (oracle/Makefile, oracle/xdrc_driver.cc).
//
//   ref_fixed <out.json>
//
// For every struct: sizeof, alignof and the offsetof of every top-level
// field (the C++ layout the staged native layout must equal), then 8
// records.  A record's storage is zeroed before the object is made in it,
// so padding bytes are zero; a seeded generator (splitmix64) fills the
// fields through the type's own xdr_traits (bools true or false, enums one
// of their tags).  Emitted: the native bytes, xdr_to_opaque of each record
// back to back, and the native bytes xdr_from_opaque makes of them in
// zeroed storage.  The two big structs give their field values instead of
// the native bytes (the opaque as a byte ramp {start, step}) and the sha256
// and first 64 bytes of the stream.  Then the reference's verdict on damaged
// streams: a nonzero pad byte, and a word that is not a tag of the validated
// enum -- the first record xdr_from_opaque throws on, the exception's class
// and its what().
#include <cinttypes>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <new>
#include <sstream>
#include <string>
#include <vector>

#include <xdrpp/marshal.h>

#include "fixedzoo.hh"
#include "ref_util.hh"

namespace fixedzoo {
template <typename T> inline void xdr_validate_enum(T);  // tests/validate.cc:18-20
}

using namespace fixedzoo;
using namespace ref_util;
using std::string;
using std::vector;

namespace {

constexpr int kRecords = 8;

// An archive that fills what it visits (xdr_traits<T>::load walks a struct's
// fields through it).
struct filler {
  rng &g;
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_numeric>::type operator()(T &t) {
    using U = typename xdr::xdr_traits<T>::uint_type;
    t = xdr::xdr_traits<T>::from_uint(U(g()));
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_enum>::type operator()(T &t) {
    const auto &v = xdr::xdr_traits<T>::enum_values();
    t = T(v[g() % v.size()]);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_bytes>::type operator()(T &t) {
    for (auto &b : t) b = uint8_t(g());
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_class>::type operator()(T &t) {
    xdr::xdr_traits<T>::load(*this, t);
  }
  template <typename T> typename std::enable_if<xdr::xdr_traits<T>::is_container>::type operator()(T &t) {
    for (auto &e : t) xdr::archive(*this, e);
  }
};

// kRecords objects of T in zeroed storage
template <typename T> struct zeroed {
  void *mem;
  zeroed() : mem(calloc(kRecords, sizeof(T))) {
    for (int r = 0; r < kRecords; ++r) new (static_cast<char *>(mem) + r * sizeof(T)) T;
  }
  ~zeroed() {
    for (int r = 0; r < kRecords; ++r) (*this)[r].~T();
    free(mem);
  }
  T &operator[](int r) { return *reinterpret_cast<T *>(static_cast<char *>(mem) + r * sizeof(T)); }
};

struct damage {
  const char *kind;  // "pad" or "enum"
  int record;
  uint32_t offset;   // in the record's wire bytes
  uint8_t value;     // pad: the byte; enum: the word's last byte (the others 0)
};

// The first record of `wire` (kRecords of them, W bytes each) the reference
// throws on.
template <typename T> string verdict(const vector<uint8_t> &wire, size_t W) {
  for (int r = 0; r < kRecords; ++r) {
    const vector<uint8_t> one(wire.begin() + r * W, wire.begin() + (r + 1) * W);
    zeroed<T> back;
    string exc;
    try {
      xdr::xdr_from_opaque(one, back[0]);
      continue;
    } catch (const xdr::xdr_should_be_zero &e) {
      exc = string("\"exception\": \"xdr_should_be_zero\", \"what\": ") + q(e.what());
    } catch (const xdr::xdr_invariant_failed &e) {
      exc = string("\"exception\": \"xdr_invariant_failed\", \"what\": ") + q(e.what());
    } catch (const std::exception &e) {
      exc = string("\"exception\": \"other\", \"what\": ") + q(e.what());
    }
    return "\"record\": " + std::to_string(r) + ", " + exc;
  }
  return "\"record\": null, \"exception\": \"none\", \"what\": \"\"";
}

template <typename T>
string emit(const char *name, const string &offs, zeroed<T> &v, const string &values,
            const vector<damage> &dmg) {
  vector<uint8_t> wire;
  size_t W = 0;
  for (int r = 0; r < kRecords; ++r) {
    const auto m = xdr::xdr_to_opaque(v[r]);
    W = m.size();
    wire.insert(wire.end(), m.begin(), m.end());
  }
  zeroed<T> back;
  for (int r = 0; r < kRecords; ++r) {
    const vector<uint8_t> one(wire.begin() + r * W, wire.begin() + (r + 1) * W);
    xdr::xdr_from_opaque(one, back[r]);
    if (memcmp(&back[r], &v[r], sizeof(T))) {  // (bytes, not ==: a float field may hold a NaN)
      fprintf(stderr, "%s: round trip mismatch\n", name);
      exit(1);
    }
  }
  std::ostringstream o;
  o << q(name) << ": {\"sizeof\": " << sizeof(T) << ", \"alignof\": " << alignof(T)
    << ", \"wire\": " << W << ",\n  \"offsetof\": {" << offs << "},\n";
  if (values.empty()) {
    o << "  \"native\": " << q(hex(v.mem, kRecords * sizeof(T))) << ",\n"
      << "  \"xdr\": " << q(hex(wire.data(), wire.size())) << ",\n"
      << "  \"decoded\": " << q(hex(back.mem, kRecords * sizeof(T))) << ",\n";
  } else {
    o << "  \"values\": [" << values << "],\n"
      << "  \"native_sha256\": " << q(sha256(static_cast<const uint8_t *>(v.mem), kRecords * sizeof(T))) << ",\n"
      << "  \"xdr_sha256\": " << q(sha256(wire.data(), wire.size())) << ",\n"
      << "  \"xdr_head\": " << q(hex(wire.data(), 64)) << ",\n"
      << "  \"decoded_sha256\": " << q(sha256(static_cast<const uint8_t *>(back.mem), kRecords * sizeof(T))) << ",\n";
  }
  o << "  \"damaged\": [";
  for (size_t k = 0; k < dmg.size(); ++k) {
    const damage &d = dmg[k];
    vector<uint8_t> bad = wire;
    uint8_t *p = bad.data() + d.record * W + d.offset;
    if (!strcmp(d.kind, "enum")) { p[0] = p[1] = p[2] = 0; p[3] = d.value; } else { p[0] = d.value; }
    o << (k ? ",\n    " : "\n    ") << "{\"kind\": " << q(d.kind) << ", \"at_record\": " << d.record
      << ", \"offset\": " << d.offset << ", \"value\": " << int(d.value) << ", " << verdict<T>(bad, W) << "}";
  }
  o << "]}";
  return o.str();
}

template <typename T> void fill(zeroed<T> &v, uint64_t seed) {
  rng g{seed};
  filler f{g};
  for (int r = 0; r < kRecords; ++r) f(v[r]);
}

#define OFF(T, f) (string("\"" #f "\": ") + std::to_string(offsetof(T, f)))
string join(std::initializer_list<string> l) {
  string s;
  for (const string &x : l) s += (s.empty() ? "" : ", ") + x;
  return s;
}

// big structs: the opaque is the ramp start + k * step (mod 256)
template <typename A> string ramp(A &o, rng &g) {
  const unsigned start = unsigned(g() & 0xff), step = unsigned(g() & 0xff) | 1u;
  for (size_t k = 0; k < o.size(); ++k) o[k] = uint8_t(start + k * step);
  return "[" + std::to_string(start) + ", " + std::to_string(step) + "]";
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: ref_fixed <out.json>\n");
    return 2;
  }
  vector<string> out;
  uint64_t seed = 0x66697865647a6f6full;
#define PLAIN(T, offs, ...)                                     \
  do {                                                          \
    zeroed<T> v;                                                \
    fill(v, ++seed);                                            \
    out.push_back(emit<T>(#T, offs, v, "", {__VA_ARGS__}));     \
  } while (0)
  PLAIN(id16_bool, join({OFF(id16_bool, a), OFF(id16_bool, i), OFF(id16_bool, b), OFF(id16_bool, j)}));
  PLAIN(id32_mix,
        join({OFF(id32_mix, b), OFF(id32_mix, i), OFF(id32_mix, o), OFF(id32_mix, j), OFF(id32_mix, e),
              OFF(id32_mix, h)}),
        damage{"pad", 5, 15, 0x80}, damage{"enum", 2, 20, 2});
  PLAIN(id48_pad,
        join({OFF(id48_pad, o), OFF(id48_pad, i), OFF(id48_pad, j), OFF(id48_pad, h), OFF(id48_pad, u),
              OFF(id48_pad, k), OFF(id48_pad, f), OFF(id48_pad, d)}),
        damage{"pad", 3, 6, 1}, damage{"pad", 6, 7, 0xff});
  PLAIN(id80_enum,
        join({OFF(id80_enum, o), OFF(id80_enum, e), OFF(id80_enum, i), OFF(id80_enum, h1), OFF(id80_enum, h2),
              OFF(id80_enum, d), OFF(id80_enum, a), OFF(id80_enum, b), OFF(id80_enum, h3), OFF(id80_enum, f),
              OFF(id80_enum, e2), OFF(id80_enum, h4), OFF(id80_enum, t0), OFF(id80_enum, t1)}),
        damage{"pad", 4, 7, 9}, damage{"enum", 1, 8, 0}, damage{"enum", 7, 60, 7});
  PLAIN(id112, join({OFF(id112, a), OFF(id112, b), OFF(id112, h), OFF(id112, c), OFF(id112, g)}));
  PLAIN(id208, join({OFF(id208, h), OFF(id208, i), OFF(id208, g)}));
  PLAIN(lastbool, join({OFF(lastbool, h), OFF(lastbool, i), OFF(lastbool, b)}));
  PLAIN(bool4, join({OFF(bool4, a), OFF(bool4, b), OFF(bool4, c), OFF(bool4, d), OFF(bool4, i)}));
  PLAIN(bytes124, join({OFF(bytes124, a), OFF(bytes124, b), OFF(bytes124, c), OFF(bytes124, i)}),
        damage{"pad", 0, 1, 1}, damage{"pad", 7, 11, 0x40});
  PLAIN(tailbools, join({OFF(tailbools, i), OFF(tailbools, a), OFF(tailbools, b)}));
  PLAIN(enumpad, join({OFF(enumpad, e), OFF(enumpad, o), OFF(enumpad, b), OFF(enumpad, f)}),
        damage{"pad", 6, 7, 3}, damage{"enum", 3, 12, 0});
  PLAIN(wide16,
        join({OFF(wide16, a), OFF(wide16, b), OFF(wide16, i), OFF(wide16, h), OFF(wide16, j), OFF(wide16, g),
              OFF(wide16, k)}));
  PLAIN(odd7, join({OFF(odd7, a), OFF(odd7, b), OFF(odd7, i)}));
  PLAIN(vpair, join({OFF(vpair, h), OFF(vpair, b)}));
  PLAIN(arr5, join({OFF(arr5, v), OFF(arr5, t)}));
#undef PLAIN
  {
    zeroed<big10k> v;
    rng g{++seed};
    string vals;
    for (int r = 0; r < kRecords; ++r) {
      const string o = ramp(v[r].o, g);
      v[r].i = int32_t(g());
      v[r].b = g() & 1;
      vals += string(r ? ", " : "") + "{\"o\": " + o + ", \"i\": " + std::to_string(v[r].i) +
              ", \"b\": " + std::to_string(int(v[r].b)) + "}";
    }
    out.push_back(emit<big10k>("big10k", join({OFF(big10k, o), OFF(big10k, i), OFF(big10k, b)}), v, vals,
                               {damage{"pad", 2, 10003, 1}}));
  }
  {
    zeroed<big20k> v;
    rng g{++seed};
    string vals;
    for (int r = 0; r < kRecords; ++r) {
      const string o = ramp(v[r].o, g);
      v[r].i = int32_t(g());
      vals += string(r ? ", " : "") + "{\"o\": " + o + ", \"i\": " + std::to_string(v[r].i) + "}";
    }
    out.push_back(emit<big20k>("big20k", join({OFF(big20k, o), OFF(big20k, i)}), v, vals,
                               {damage{"pad", 5, 20001, 0x10}}));
  }

  std::ofstream f(argv[1]);
  f << "{\"generator\": \"oracle/ref_fixed.cc over genuine xdrc output of oracle/x/fixedzoo.x\",\n"
    << "\"records\": " << kRecords << ",\n\"structs\": {\n";
  for (size_t k = 0; k < out.size(); ++k) f << out[k] << (k + 1 < out.size() ? ",\n" : "\n");
  f << "}\n}\n";
  f.close();
  return f ? 0 : 1;
}
