// Stand-alone driver of the library's HOST code, for tests/test_host_sanitized_cpu.py.  It is linked against the library's translation
// units compiled from source with the host side under a sanitizer (tests/host_driver_build.py); it is never loaded into an interpreter
// and never goes through dlopen.
//
//   host_driver <command> <directory>
//
// reads its inputs from <directory> (raw little-endian arrays and small text tables the pytest side writes), calls the C ABI and writes
// its outputs beside them.  Exit status 0: every check the driver makes itself held.  Every buffer handed to the library is a heap
// allocation of exactly the documented size, so a sanitizer's red zone sits right behind the last element.  Only entry points, and
// refusal paths of entry points, that return before any HIP runtime call are used.
#include <pthread.h>

#include <cerrno>
#include <cinttypes>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "linetr_hip.h"

namespace {

std::string g_dir;
int g_failures = 0;

[[noreturn]] void die(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "host_driver: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  exit(2);
}
void mismatch(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "host_driver MISMATCH: ");
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  ++g_failures;
}
#define CHECK(cond, ...) do { if (!(cond)) mismatch(__VA_ARGS__); } while (0)

// an exact-size heap allocation: n elements and not a byte more
template <class T> struct Heap {
  T* p = nullptr;
  size_t n = 0;
  Heap() = default;
  explicit Heap(size_t n_, int fill = 0) : p((T*)malloc(n_ * sizeof(T))), n(n_) {
    if (n_ && !p) die("out of memory");
    if (n_) memset((void*)p, fill, n_ * sizeof(T));
  }
  Heap(Heap&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  Heap& operator=(Heap&& o) noexcept { if (this != &o) { free(p); p = o.p; n = o.n; o.p = nullptr; o.n = 0; } return *this; }
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
  ~Heap() { free(p); }
  size_t bytes() const { return n * sizeof(T); }
  bool all_bytes(int v) const {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < bytes(); ++i) if (b[i] != (unsigned char)v) return false;
    return true;
  }
};

std::string path(const std::string& name) { return g_dir + "/" + name; }
bool exists(const std::string& name) { return std::ifstream(path(name)).good(); }

template <class T> Heap<T> read_bin(const std::string& name) {
  FILE* f = fopen(path(name).c_str(), "rb");
  if (!f) die("cannot read %s", path(name).c_str());
  fseek(f, 0, SEEK_END);
  const long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  if (sz < 0 || sz % (long)sizeof(T)) die("%s: %ld bytes is no array of %zu-byte elements", name.c_str(), sz, sizeof(T));
  Heap<T> h((size_t)sz / sizeof(T));
  if (sz && fread((void*)h.p, 1, (size_t)sz, f) != (size_t)sz) die("short read of %s", name.c_str());
  fclose(f);
  return h;
}
void write_bin(const std::string& name, const void* p, size_t bytes) {
  FILE* f = fopen(path(name).c_str(), "wb");
  if (!f) die("cannot write %s", path(name).c_str());
  if (bytes && fwrite(p, 1, bytes, f) != bytes) die("short write of %s", name.c_str());
  fclose(f);
}
std::vector<std::vector<std::string>> read_table(const std::string& name) {
  std::ifstream in(path(name));
  if (!in) die("cannot read %s", path(name).c_str());
  std::vector<std::vector<std::string>> rows;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::vector<std::string> row;
    std::string w;
    while (ss >> w) row.push_back(w);
    if (!row.empty()) rows.push_back(row);
  }
  return rows;
}
int64_t to_i64(const std::string& s) { return strtoll(s.c_str(), nullptr, 10); }
double to_f64(const std::string& s) { return strtod(s.c_str(), nullptr); }   // repr() of a Python float round-trips

const char* last_error() { return linetr_last_error(); }
// leaves a known text in the calling thread's error slot, so that a refusal that sets none shows
void stale_error() { (void)linetr_set_precision(nullptr, 0); }
const char* const STALE = "bad precision mode";

// ============================================================================================================================
// prefilter
// ============================================================================================================================

struct PfCase {
  std::string id;
  int B, height, width, border, max_keylines, T, expect;
  double min_length, td;
  Heap<double> lines;
  Heap<int32_t> off;
  std::vector<Heap<double>> vm;      // per image; n == 0: none
  Heap<const double*> vm_ptrs;       // exactly B pointers, or none at all
  bool any_vm = false;
};

PfCase load_pf_case(const std::vector<std::string>& r) {
  if (r.size() != 10) die("cases.txt: a row has %zu fields, not 10", r.size());
  PfCase c;
  c.id = r[0];
  c.B = (int)to_i64(r[1]); c.height = (int)to_i64(r[2]); c.width = (int)to_i64(r[3]); c.border = (int)to_i64(r[4]);
  c.min_length = to_f64(r[5]); c.max_keylines = (int)to_i64(r[6]); c.td = to_f64(r[7]); c.T = (int)to_i64(r[8]); c.expect = (int)to_i64(r[9]);
  c.lines = read_bin<double>(c.id + "_lines.bin");
  c.off = read_bin<int32_t>(c.id + "_off.bin");
  if ((int)c.off.n != c.B + 1 || c.lines.n != (size_t)c.off.p[c.B] * 6) die("case %s: offsets and lines disagree", c.id.c_str());
  c.vm.resize(c.B);
  for (int i = 0; i < c.B; ++i)
    if (exists(c.id + "_vm" + std::to_string(i) + ".bin")) {
      c.vm[i] = read_bin<double>(c.id + "_vm" + std::to_string(i) + ".bin");
      if (c.vm[i].n != (size_t)c.height * c.width) die("case %s: valid mask %d has the wrong size", c.id.c_str(), i);
      c.any_vm = true;
    }
  if (c.any_vm) {
    c.vm_ptrs = Heap<const double*>(c.B);
    for (int i = 0; i < c.B; ++i) c.vm_ptrs.p[i] = c.vm[i].n ? c.vm[i].p : nullptr;
  }
  return c;
}

struct PfResult { int code = 0; Heap<LinetrLineRec> recs; Heap<int32_t> cu_k, cu_n, tied; };

// one linetr_prefilter_batch call into exact-size buffers (records: `capacity` of them), then the tied images of that call
PfResult pf_batch(const PfCase& c, int n_threads, int capacity) {
  PfResult r;
  r.recs = Heap<LinetrLineRec>((size_t)capacity, 0xAB);
  r.cu_k = Heap<int32_t>((size_t)c.B + 1, 0xCD);
  r.cu_n = Heap<int32_t>((size_t)c.B + 1, 0xCD);
  r.code = linetr_prefilter_batch(c.lines.p, c.off.p, c.B, c.height, c.width, c.border, c.min_length, c.max_keylines,
                                  c.any_vm ? c.vm_ptrs.p : nullptr, c.td, c.T, n_threads, r.recs.p, capacity, r.cu_k.p, r.cu_n.p);
  if (r.code == LINETR_OK) {
    const int32_t n = linetr_prefilter_tied_images(nullptr, 0);
    r.tied = Heap<int32_t>((size_t)n, 0xEE);
    if (linetr_prefilter_tied_images(r.tied.p, n) != n) mismatch("case %s: the tied-image count changed between two reads", c.id.c_str());
  }
  return r;
}

bool same_result(const PfResult& a, const PfResult& b, size_t k) {
  return a.code == b.code && a.cu_k.bytes() == b.cu_k.bytes() && !memcmp(a.cu_k.p, b.cu_k.p, a.cu_k.bytes()) &&
         !memcmp(a.cu_n.p, b.cu_n.p, a.cu_n.bytes()) && (k == 0 || !memcmp(a.recs.p, b.recs.p, k * sizeof(LinetrLineRec))) &&
         a.tied.n == b.tied.n && (a.tied.n == 0 || !memcmp(a.tied.p, b.tied.p, a.tied.bytes()));
}

int cmd_prefilter() {
  static const int THREADS[] = {0, 1, 2, 8};
  for (const auto& row : read_table("cases.txt")) {
    const PfCase c = load_pf_case(row);
    const int K = c.off.p[c.B];
    const PfResult ref = pf_batch(c, 1, K);
    CHECK(ref.code == c.expect, "case %s: status %d, expected %d (%s)", c.id.c_str(), ref.code, c.expect, last_error());
    if (c.expect != LINETR_OK) {
      CHECK(last_error()[0] != 0, "case %s: a refusal without a message", c.id.c_str());
      for (int nt : THREADS) CHECK(pf_batch(c, nt, K).code == c.expect, "case %s: n_threads %d does not give status %d", c.id.c_str(), nt, c.expect);
      continue;
    }
    if (ref.code != LINETR_OK) continue;
    const int k = ref.cu_k.p[c.B];
    for (int nt : THREADS) {                                          // exact capacity: every thread setting, the same bytes
      const PfResult got = pf_batch(c, nt, k);
      CHECK(same_result(ref, got, (size_t)k), "case %s: n_threads %d differs from n_threads 1", c.id.c_str(), nt);
    }
    if (k > 0)
      for (int nt : THREADS) {                                        // one record short
        const PfResult got = pf_batch(c, nt, k - 1);
        CHECK(got.code == LINETR_E_CAPACITY, "case %s: capacity %d with n_threads %d gave %d, not LINETR_E_CAPACITY", c.id.c_str(), k - 1, nt, got.code);
      }
    write_bin(c.id + "_recs.bin", ref.recs.p, (size_t)k * sizeof(LinetrLineRec));
    write_bin(c.id + "_cu_k.bin", ref.cu_k.p, ref.cu_k.bytes());
    write_bin(c.id + "_cu_n.bin", ref.cu_n.p, ref.cu_n.bytes());
    write_bin(c.id + "_tied.bin", ref.tied.p, ref.tied.bytes());
    if (c.B != 1) continue;
    // one image: linetr_prefilter gives the batch's records, and linetr_pack_lines re-packs them to the same bytes
    Heap<LinetrLineRec> one((size_t)k, 0xAB);
    int32_t k_out = -1, n_out = -1;
    int code = linetr_prefilter(c.lines.p, K, c.height, c.width, c.border, c.min_length, c.max_keylines, c.vm[0].n ? c.vm[0].p : nullptr, c.td, c.T,
                                0, 0, 0, one.p, k, &k_out, &n_out);
    CHECK(code == LINETR_OK && k_out == k && n_out == ref.cu_n.p[1] && (k == 0 || !memcmp(one.p, ref.recs.p, one.bytes())),
          "case %s: linetr_prefilter differs from the batch of one (status %d, %d lines)", c.id.c_str(), code, k_out);
    Heap<int32_t> tied(1, 0xEE);
    const int32_t n_tied = linetr_prefilter_tied_images(tied.p, 1);
    CHECK(n_tied == (int32_t)ref.tied.n && (n_tied == 0 || tied.p[0] == 0), "case %s: linetr_prefilter reports %d tied images", c.id.c_str(), n_tied);
    if (k > 0) {
      Heap<LinetrLineRec> shorter((size_t)k - 1, 0xAB);
      code = linetr_prefilter(c.lines.p, K, c.height, c.width, c.border, c.min_length, c.max_keylines, c.vm[0].n ? c.vm[0].p : nullptr, c.td, c.T, 0,
                              0, 0, shorter.p, k - 1, &k_out, &n_out);
      CHECK(code == LINETR_E_CAPACITY, "case %s: linetr_prefilter with capacity %d gave %d", c.id.c_str(), k - 1, code);
    }
    Heap<double> kl((size_t)k * 4), len((size_t)k), ang((size_t)k * 2);
    for (int i = 0; i < k; ++i) {
      memcpy(kl.p + 4 * i, ref.recs.p[i].sp, 16); memcpy(kl.p + 4 * i + 2, ref.recs.p[i].ep, 16);
      len.p[i] = ref.recs.p[i].length;
      memcpy(ang.p + 2 * i, ref.recs.p[i].angle, 16);
    }
    Heap<LinetrLineRec> packed((size_t)k, 0xAB);
    int32_t n_packed = -1;
    code = linetr_pack_lines(kl.p, len.p, ang.p, k, c.td, c.T, 0, 0, 0, packed.p, &n_packed);
    CHECK(code == LINETR_OK && n_packed == ref.cu_n.p[1] && (k == 0 || !memcmp(packed.p, ref.recs.p, packed.bytes())),
          "case %s: linetr_pack_lines differs from the pre-filter's records (status %d)", c.id.c_str(), code);
  }
  return 0;
}

// ============================================================================================================================
// pseudo lines
// ============================================================================================================================

int cmd_pseudo() {
  // cases.txt: id seed image n shape0 shape1 min_length max_sublines
  for (const auto& r : read_table("cases.txt")) {
    if (r.size() != 8) die("cases.txt: a row has %zu fields, not 8", r.size());
    const std::string id = r[0];
    const uint64_t seed = (uint64_t)to_i64(r[1]);
    const int image = (int)to_i64(r[2]), n = (int)to_i64(r[3]), max_sub = (int)to_i64(r[7]);
    const double s0 = to_f64(r[4]), s1 = to_f64(r[5]), min_length = to_f64(r[6]);
    Heap<double> lines((size_t)n * 4, 0xAB);
    int code = linetr_make_pseudo_lines(seed, image, n, s0, s1, min_length, lines.p);
    CHECK(code == LINETR_OK, "case %s: make_pseudo_lines gave %d (%s)", id.c_str(), code, last_error());
    Heap<double> kl((size_t)n * 4, 0xAB), len((size_t)n, 0xAB), ang((size_t)n * 2, 0xAB);
    Heap<int32_t> n_out(1, 0xEE);
    code = linetr_find_line_attributes(lines.p, n, min_length, max_sub, kl.p, len.p, ang.p, n_out.p);
    CHECK(code == LINETR_OK && n_out.p[0] >= 0 && n_out.p[0] <= n, "case %s: find_line_attributes gave %d, %d rows (%s)", id.c_str(), code, n_out.p[0], last_error());
    write_bin(id + "_lines.bin", lines.p, lines.bytes());
    write_bin(id + "_klines.bin", kl.p, kl.bytes());
    write_bin(id + "_length.bin", len.p, len.bytes());
    write_bin(id + "_angles.bin", ang.p, ang.bytes());
    write_bin(id + "_n.bin", n_out.p, 4);
  }
  return 0;
}

// ============================================================================================================================
// weight preparation
// ============================================================================================================================

int cmd_prepare() {
  // cfg.bin: the LinetrModelConfig; names.txt: one state-dict key per line; t<i>.bin: tensor i, float32
  const Heap<LinetrModelConfig> cfg = read_bin<LinetrModelConfig>("cfg.bin");
  if (cfg.n != 1) die("cfg.bin holds %zu configurations", cfg.n);
  const auto rows = read_table("names.txt");
  const int n = (int)rows.size();
  std::vector<Heap<char>> names(n);
  std::vector<Heap<float>> data(n);
  Heap<const char*> name_ptrs((size_t)n);
  Heap<const float*> data_ptrs((size_t)n);
  Heap<int64_t> numel((size_t)n);
  for (int i = 0; i < n; ++i) {
    names[i] = Heap<char>(rows[i][0].size() + 1);
    memcpy(names[i].p, rows[i][0].c_str(), rows[i][0].size() + 1);
    data[i] = read_bin<float>("t" + std::to_string(i) + ".bin");
    name_ptrs.p[i] = names[i].p; data_ptrs.p[i] = data[i].p; numel.p[i] = (int64_t)data[i].n;
  }
  Heap<int64_t> nf(1); Heap<int32_t> ne(1);
  nf.p[0] = -1; ne.p[0] = -1;
  int code = linetr_debug_prepare(cfg.p, n, name_ptrs.p, data_ptrs.p, numel.p, nullptr, 0, nullptr, 0, nf.p, ne.p);
  if (code != LINETR_OK || nf.p[0] <= 0 || ne.p[0] <= 0) { mismatch("the size call gave %d, %lld floats, %d entries (%s)", code, (long long)nf.p[0], ne.p[0], last_error()); return 0; }
  const int64_t floats = nf.p[0];
  const int32_t entries = ne.p[0];
  Heap<float> image((size_t)floats, 0xAB);
  Heap<LinetrPreparedEntry> table((size_t)entries, 0xAB);
  code = linetr_debug_prepare(cfg.p, n, name_ptrs.p, data_ptrs.p, numel.p, image.p, floats, table.p, entries, nf.p, ne.p);
  CHECK(code == LINETR_OK && nf.p[0] == floats && ne.p[0] == entries, "exact capacities gave %d (%s)", code, last_error());
  write_bin("image.bin", image.p, image.bytes());
  write_bin("table.bin", table.p, table.bytes());
  {   // one float short, and one entry short: refused, sizes reported, nothing written
    Heap<float> image1((size_t)floats - 1, 0xAB);
    Heap<LinetrPreparedEntry> table1((size_t)entries, 0xAB);
    code = linetr_debug_prepare(cfg.p, n, name_ptrs.p, data_ptrs.p, numel.p, image1.p, floats - 1, table1.p, entries, nf.p, ne.p);
    CHECK(code == LINETR_E_CAPACITY && nf.p[0] == floats && ne.p[0] == entries && image1.all_bytes(0xAB) && table1.all_bytes(0xAB),
          "an image one float short gave %d (%s)", code, last_error());
    Heap<float> image2((size_t)floats, 0xAB);
    Heap<LinetrPreparedEntry> table2((size_t)entries - 1, 0xAB);
    code = linetr_debug_prepare(cfg.p, n, name_ptrs.p, data_ptrs.p, numel.p, image2.p, floats, table2.p, entries - 1, nf.p, ne.p);
    CHECK(code == LINETR_E_CAPACITY && nf.p[0] == floats && ne.p[0] == entries && image2.all_bytes(0xAB) && table2.all_bytes(0xAB),
          "a table one entry short gave %d (%s)", code, last_error());
  }
  {   // either buffer alone, and the same bytes again
    Heap<float> image3((size_t)floats, 0xAB);
    code = linetr_debug_prepare(cfg.p, n, name_ptrs.p, data_ptrs.p, numel.p, image3.p, floats, nullptr, 0, nf.p, ne.p);
    CHECK(code == LINETR_OK && !memcmp(image3.p, image.p, image.bytes()), "the image alone gave %d or other bytes", code);
    Heap<LinetrPreparedEntry> table3((size_t)entries, 0xAB);
    code = linetr_debug_prepare(cfg.p, n, name_ptrs.p, data_ptrs.p, numel.p, nullptr, 0, table3.p, entries, nf.p, ne.p);
    CHECK(code == LINETR_OK && !memcmp(table3.p, table.p, table.bytes()), "the table alone gave %d or other bytes", code);
  }
  return 0;
}

// ============================================================================================================================
// photometric sampler
// ============================================================================================================================

int cmd_photo() {
  // cases.txt: id seed first B H W expect; <id>_cfg.bin: the LinetrPhotoConfig
  for (const auto& r : read_table("cases.txt")) {
    if (r.size() != 7) die("cases.txt: a row has %zu fields, not 7", r.size());
    const std::string id = r[0];
    const Heap<LinetrPhotoConfig> cfg = read_bin<LinetrPhotoConfig>(id + "_cfg.bin");
    if (cfg.n != 1) die("%s_cfg.bin holds %zu configurations", id.c_str(), cfg.n);
    const int B = (int)to_i64(r[3]), expect = (int)to_i64(r[6]);
    Heap<LinetrPhotoParams> out((size_t)std::max(B, 0), 0);
    const int code = linetr_photometric_sample(cfg.p, (uint64_t)to_i64(r[1]), (int)to_i64(r[2]), B, (int)to_i64(r[4]), (int)to_i64(r[5]), out.p);
    CHECK(code == expect, "case %s: status %d, expected %d (%s)", id.c_str(), code, expect, last_error());
    if (expect != LINETR_OK) CHECK(out.all_bytes(0) && last_error()[0] != 0, "case %s: a refused call wrote parameters or left no message", id.c_str());
    write_bin(id + "_params.bin", out.p, out.bytes());
  }
  return 0;
}

// ============================================================================================================================
// size queries
// ============================================================================================================================

struct Query {
  const char* name;
  std::vector<int> width;       // per argument: 32 or 64 (bits); 1: a flag (0 / 1)
  std::vector<int64_t> base;    // a small shape the entry point serves
  int n_offsets;                // int64 offsets written behind the arguments (0: none)
  std::function<int64_t(const int64_t*, int64_t*)> call;
};
#define I(k) ((int32_t)a[k])
const std::vector<Query>& queries() {
  static const std::vector<Query> q = {
      {"linetr_tokenize_workspace_bytes", {32, 32, 32, 32}, {2, 64, 96, 37}, 0, [](const int64_t* a, int64_t*) { return linetr_tokenize_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_sample_descriptors_workspace_bytes", {32, 32, 1}, {8, 12, 0}, 0, [](const int64_t* a, int64_t*) { return linetr_sample_descriptors_workspace_bytes(I(0), I(1), I(2)); }},
      {"linetr_point_descriptors_workspace_bytes", {32, 32, 32, 1}, {2, 8, 12, 0}, 0, [](const int64_t* a, int64_t*) { return linetr_point_descriptors_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_match_workspace_bytes", {32, 64, 64, 64}, {2, 3088, 900, 146}, 0, [](const int64_t* a, int64_t*) { return linetr_match_workspace_bytes(I(0), a[1], a[2], a[3]); }},
      {"linetr_match_distmat_workspace_bytes", {32, 32}, {17, 64}, 0, [](const int64_t* a, int64_t*) { return linetr_match_distmat_workspace_bytes(I(0), I(1)); }},
      {"linetr_match_distmat_f64_workspace_bytes", {32, 32}, {17, 64}, 0, [](const int64_t* a, int64_t*) { return linetr_match_distmat_f64_workspace_bytes(I(0), I(1)); }},
      {"linetr_pool_distmat_workspace_bytes", {32, 32}, {17, 64}, 0, [](const int64_t* a, int64_t*) { return linetr_pool_distmat_workspace_bytes(I(0), I(1)); }},
      {"linetr_pool_distmat_dense_workspace_bytes", {32, 32, 32, 32}, {30, 40, 35, 50}, 0, [](const int64_t* a, int64_t*) { return linetr_pool_distmat_dense_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_match_points_workspace_bytes", {32, 32}, {33, 31}, 0, [](const int64_t* a, int64_t*) { return linetr_match_points_workspace_bytes(I(0), I(1)); }},
      {"linetr_pair_tail_workspace_bytes", {32, 32, 32, 32, 32, 32}, {33, 31, 40, 30, 50, 35}, 0, [](const int64_t* a, int64_t*) { return linetr_pair_tail_workspace_bytes(I(0), I(1), I(2), I(3), I(4), I(5)); }},
      {"linetr_pair_tail_output_bytes", {32, 32, 32, 32}, {33, 31, 30, 35}, 4, [](const int64_t* a, int64_t* o) { return linetr_pair_tail_output_bytes(I(0), I(1), I(2), I(3), o); }},
      {"linetr_val_step_workspace_bytes", {32, 32}, {4, 128}, 0, [](const int64_t* a, int64_t*) { return linetr_val_step_workspace_bytes(I(0), I(1)); }},
      {"linetr_val_step_output_bytes", {32}, {4}, 4, [](const int64_t* a, int64_t* o) { return linetr_val_step_output_bytes(I(0), o); }},
      {"linetr_desc_loss_grad_workspace_bytes", {32, 32}, {4, 128}, 0, [](const int64_t* a, int64_t*) { return linetr_desc_loss_grad_workspace_bytes(I(0), I(1)); }},
      {"linetr_linear_backward_workspace_bytes", {64, 32, 32}, {100, 256, 256}, 0, [](const int64_t* a, int64_t*) { return linetr_linear_backward_workspace_bytes(a[0], I(1), I(2)); }},
      {"linetr_head_backward_workspace_bytes", {64}, {100}, 0, [](const int64_t* a, int64_t*) { return linetr_head_backward_workspace_bytes(a[0]); }},
      {"linetr_sig_attention_backward_workspace_bytes", {64}, {100}, 0, [](const int64_t* a, int64_t*) { return linetr_sig_attention_backward_workspace_bytes(a[0]); }},
      {"linetr_bn_forward_workspace_bytes", {64, 32}, {100, 256}, 0, [](const int64_t* a, int64_t*) { return linetr_bn_forward_workspace_bytes(a[0], I(1)); }},
      {"linetr_bn_backward_workspace_bytes", {64, 32}, {100, 256}, 0, [](const int64_t* a, int64_t*) { return linetr_bn_backward_workspace_bytes(a[0], I(1)); }},
      {"linetr_layer_norm_backward_workspace_bytes", {64, 32}, {100, 256}, 0, [](const int64_t* a, int64_t*) { return linetr_layer_norm_backward_workspace_bytes(a[0], I(1)); }},
      {"linetr_input_layer_backward_workspace_bytes", {64, 32, 32}, {100, 32, 4}, 0, [](const int64_t* a, int64_t*) { return linetr_input_layer_backward_workspace_bytes(a[0], I(1), I(2)); }},
      {"linetr_token_assemble_backward_workspace_bytes", {64}, {100}, 0, [](const int64_t* a, int64_t*) { return linetr_token_assemble_backward_workspace_bytes(a[0]); }},
      {"linetr_gt_assign_workspace_bytes", {32, 32, 32}, {4, 128, 128}, 0, [](const int64_t* a, int64_t*) { return linetr_gt_assign_workspace_bytes(I(0), I(1), I(2)); }},
      {"linetr_fixed_size_workspace_bytes", {32, 32, 32, 1}, {4, 64, 96, 0}, 0, [](const int64_t* a, int64_t*) { return linetr_fixed_size_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_adam_workspace_bytes", {32, 64}, {8, 100000}, 0, [](const int64_t* a, int64_t*) { return linetr_adam_workspace_bytes(I(0), a[1]); }},
      {"linetr_grad_norm_workspace_bytes", {32, 64}, {8, 100000}, 0, [](const int64_t* a, int64_t*) { return linetr_grad_norm_workspace_bytes(I(0), a[1]); }},
      {"linetr_superpoint_keypoints_workspace_bytes", {32, 32, 32, 32}, {2, 64, 96, 400}, 0, [](const int64_t* a, int64_t*) { return linetr_superpoint_keypoints_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_photometric_workspace_bytes", {32, 32, 32, 32}, {3, 1, 33, 65}, 0, [](const int64_t* a, int64_t*) { return linetr_photometric_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_detect_lines_workspace_bytes", {32, 32, 32, 32}, {2, 64, 96, 2}, 0, [](const int64_t* a, int64_t*) { return linetr_detect_lines_workspace_bytes(I(0), I(1), I(2), I(3)); }},
      {"linetr_detect_debug_labels_workspace_bytes", {32, 32, 32}, {2, 64, 96}, 0, [](const int64_t* a, int64_t*) { return linetr_detect_debug_labels_workspace_bytes(I(0), I(1), I(2)); }},
      {"linetr_sp_conv3x3_pack_bytes", {32, 32}, {64, 128}, 0, [](const int64_t* a, int64_t*) { return linetr_sp_conv3x3_pack_bytes(I(0), I(1)); }},
      {"linetr_sp_encoder_workspace_bytes", {32, 32, 32}, {2, 64, 96}, 0, [](const int64_t* a, int64_t*) { return linetr_sp_encoder_workspace_bytes(I(0), I(1), I(2)); }},
  };
  return q;
}
#undef I

void print_query(FILE* f, const Query& q, const std::vector<int64_t>& args) {
  Heap<int64_t> offs((size_t)q.n_offsets);     // exactly the offsets the header documents
  const int64_t v = q.call(args.data(), q.n_offsets ? offs.p : nullptr);
  fprintf(f, "%s", q.name);
  for (int64_t a : args) fprintf(f, " %" PRId64, a);
  fprintf(f, " = %" PRId64, v);
  for (int i = 0; i < q.n_offsets; ++i) fprintf(f, " %" PRId64, offs.p[i]);
  fprintf(f, "\n");
  if (q.n_offsets) {                           // the offsets are optional
    const int64_t v2 = q.call(args.data(), nullptr);
    CHECK(v2 == v, "%s answers %lld with offsets and %lld without", q.name, (long long)v, (long long)v2);
  }
}

// the values around which an argument's arithmetic changes width: 2^15, 2^16, 2^31 - 1, 2^31 / (element size) of the products the layouts
// form (4-, 8-, 16-byte elements, rows of 64 .. 1024 floats, the 1224-byte parameter record, 80-byte line records), INT64_MAX
std::vector<int64_t> edge_values(int width) {
  std::vector<int64_t> v = {0, 1, -1, INT32_MIN, (1 << 15) - 1, 1 << 15, (1 << 15) + 1, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, INT32_MAX - 1, INT32_MAX};
  for (int64_t e : {2, 4, 8, 12, 16, 32, 64, 80, 256, 512, 1024, 1224, 2048, 4096, 65536})
    for (int64_t d : {-1, 0, 1}) v.push_back((int64_t(1) << 31) / e + d);
  if (width == 64) {
    v.push_back(int64_t(1) << 31); v.push_back(int64_t(1) << 32); v.push_back(INT64_MAX); v.push_back(INT64_MAX - 1); v.push_back(INT64_MIN);
    for (int64_t e : {2, 4, 8, 16, 64, 256, 1024, 4096})
      for (int64_t d : {-1, 0, 1}) v.push_back(INT64_MAX / e + d);
  }
  return v;
}

int cmd_queries() {
  // calls.txt: name and arguments per line (the pinned grids of the CPU tests) -> calls_out.txt
  FILE* f = fopen(path("calls_out.txt").c_str(), "w");
  if (!f) die("cannot write calls_out.txt");
  for (const auto& r : read_table("calls.txt")) {
    const Query* q = nullptr;
    for (const Query& c : queries()) if (r[0] == c.name) q = &c;
    if (!q || r.size() != q->width.size() + 1) die("calls.txt: no query %s of %zu arguments", r[0].c_str(), r.size() - 1);
    std::vector<int64_t> args;
    for (size_t i = 1; i < r.size(); ++i) args.push_back(to_i64(r[i]));
    print_query(f, *q, args);
  }
  fclose(f);
  // the edges: every argument separately around its base shape, then all of them together -> edges_out.txt
  f = fopen(path("edges_out.txt").c_str(), "w");
  if (!f) die("cannot write edges_out.txt");
  for (const Query& q : queries()) {
    print_query(f, q, q.base);
    for (size_t k = 0; k < q.width.size(); ++k) {
      if (q.width[k] == 1) { std::vector<int64_t> a = q.base; a[k] = 1; print_query(f, q, a); continue; }
      for (int64_t v : edge_values(q.width[k])) { std::vector<int64_t> a = q.base; a[k] = v; print_query(f, q, a); }
    }
    for (int64_t v : {int64_t(0), int64_t(-1), int64_t(INT32_MIN), int64_t(1) << 15, int64_t(1) << 16, int64_t(1) << 20, int64_t(INT32_MAX), INT64_MAX, INT64_MIN}) {
      std::vector<int64_t> a = q.base;
      for (size_t k = 0; k < a.size(); ++k)
        if (q.width[k] != 1) a[k] = q.width[k] == 64 ? v : std::max<int64_t>(INT32_MIN, std::min<int64_t>(INT32_MAX, v));
      print_query(f, q, a);
    }
  }
  fclose(f);
  // tiles and the slot count -> tiles_out.txt; a NULL pointer is refused
  f = fopen(path("tiles_out.txt").c_str(), "w");
  if (!f) die("cannot write tiles_out.txt");
  Heap<int32_t> t(8, 0xEE);
  int32_t* p = t.p;
  CHECK(linetr_warp_tile(p, p + 1, p + 2, p + 3) == LINETR_OK, "linetr_warp_tile failed");
  fprintf(f, "linetr_warp_tile %d %d %d %d\n", p[0], p[1], p[2], p[3]);
  CHECK(linetr_photometric_tile(p, p + 1, p + 2, p + 3, p + 4, p + 5, p + 6, p + 7) == LINETR_OK, "linetr_photometric_tile failed");
  fprintf(f, "linetr_photometric_tile %d %d %d %d %d %d %d %d\n", p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7]);
  CHECK(linetr_detect_tile(p, p + 1) == LINETR_OK, "linetr_detect_tile failed");
  fprintf(f, "linetr_detect_tile %d %d\n", p[0], p[1]);
  CHECK(linetr_sp_conv3x3_tile(p, p + 1) == LINETR_OK, "linetr_sp_conv3x3_tile failed");
  fprintf(f, "linetr_sp_conv3x3_tile %d %d\n", p[0], p[1]);
  fprintf(f, "linetr_pipeline_max_slots %d\n", linetr_pipeline_max_slots());
  fprintf(f, "linetr_abi_version %d\n", linetr_abi_version());
  fclose(f);
  CHECK(linetr_warp_tile(nullptr, p, p, p) == LINETR_E_ARG && linetr_warp_tile(p, p, p, nullptr) == LINETR_E_ARG, "linetr_warp_tile takes a NULL pointer");
  CHECK(linetr_photometric_tile(nullptr, p, p, p, p, p, p, p) == LINETR_E_ARG && linetr_photometric_tile(p, p, p, p, p, p, p, nullptr) == LINETR_E_ARG,
        "linetr_photometric_tile takes a NULL pointer");
  CHECK(linetr_detect_tile(nullptr, p) == LINETR_E_ARG && linetr_detect_tile(p, nullptr) == LINETR_E_ARG, "linetr_detect_tile takes a NULL pointer");
  CHECK(linetr_sp_conv3x3_tile(nullptr, p) == LINETR_E_ARG && linetr_sp_conv3x3_tile(p, nullptr) == LINETR_E_ARG, "linetr_sp_conv3x3_tile takes a NULL pointer");
  return 0;
}

// ============================================================================================================================
// refusals and malformed arguments: a table of calls, each with the status it must return
// ============================================================================================================================

struct Refusal { std::string name; int expect; std::function<int()> call; };

// runs the table, writes "<name> <status> <message>" per call to `out`
void run_refusals(const std::vector<Refusal>& table, const char* out) {
  FILE* f = fopen(path(out).c_str(), "w");
  if (!f) die("cannot write %s", out);
  for (const Refusal& r : table) {
    stale_error();
    const int code = r.call();
    const std::string msg = code == LINETR_OK ? "" : last_error();
    CHECK(code == r.expect, "%s: status %d, expected %d (%s)", r.name.c_str(), code, r.expect, msg.c_str());
    if (r.expect != LINETR_OK) CHECK(!msg.empty() && msg != STALE, "%s: refused without a message of its own", r.name.c_str());
    fprintf(f, "%s %d %s\n", r.name.c_str(), code, msg.c_str());
  }
  fclose(f);
}

int cmd_refusals() {
  // "Device" pointers: addresses inside one 256-aligned host block that no refused call may touch (it is checked to stay zero).
  Heap<unsigned char> block(8192 + 256);
  const uintptr_t p0 = ((uintptr_t)block.p + 255) / 256 * 256;
  auto q = [&](int i) { return (void*)(p0 + 256 * (uintptr_t)i); };
  auto qf = [&](int i) { return (float*)q(i); };
  auto qi = [&](int i) { return (int32_t*)q(i); };
  auto odd = [&](int i) { return (float*)(p0 + 256 * (uintptr_t)i + 4); };     // 4-byte but not 16-byte aligned
  Heap<int64_t> zero(1);
  Heap<int32_t> dims(4);
  dims.p[0] = 40; dims.p[1] = 30; dims.p[2] = 50; dims.p[3] = 35;
  const int64_t* z = zero.p;
  const int64_t need_match = linetr_match_workspace_bytes(1, 40 * 50, 0, 30 + 35);
  const int64_t out_bytes = linetr_pair_tail_output_bytes(33, 31, 30, 35, nullptr);
  LinetrTokens tok{};
  tok.klines = qf(0); tok.length = qf(1); tok.angles = qf(2); tok.sublines = qf(3); tok.pnt = qf(4); tok.mask = qf(5); tok.resp = qf(6);
  tok.angle_sub = qf(7); tok.desc = qf(8); tok.score = qf(9);
  const LinetrLineRec* recs = (const LinetrLineRec*)q(10);
  const int W = LINETR_E_WORKSPACE, A = LINETR_E_ARG, Cp = LINETR_E_CAPACITY;
  std::vector<Refusal> t = {
      // a workspace one byte short of the query's answer
      {"match/short", W, [&] { return linetr_match(nullptr, 1, dims.p, qf(0), z, qi(1), qf(2), z, qi(3), 0.8f, 1, qf(4), z, qi(5), z, q(6), need_match - 1, nullptr); }},
      {"match_gathered/short", W, [&] { return linetr_match_gathered(nullptr, 1, dims.p, qf(0), z, qi(1), z, qf(2), z, qi(3), z, 0.8f, 1, qf(4), z, qi(5), z, q(6), need_match - 1, nullptr); }},
      {"match_points/short", W, [&] { return linetr_match_points(nullptr, qf(0), 33, qf(1), 31, 0.8f, 1, qf(2), qi(3), q(4), linetr_match_points_workspace_bytes(33, 31) - 1, nullptr); }},
      {"pair_tail/short", W, [&] { return linetr_pair_tail(nullptr, qf(0), 33, qf(1), 31, 0.7f, qf(2), 40, qi(3), 30, qf(4), 50, qi(5), 35, 0.8f, 1, q(6), out_bytes, q(7),
                                                           linetr_pair_tail_workspace_bytes(33, 31, 40, 30, 50, 35) - 1, nullptr); }},
      {"match_distmat/short", W, [&] { return linetr_match_distmat(nullptr, qf(0), 17, 64, 0.8f, 1, qi(1), q(2), linetr_match_distmat_workspace_bytes(17, 64) - 1, nullptr); }},
      {"match_distmat_f64/short", W, [&] { return linetr_match_distmat_f64(nullptr, (const double*)q(0), 5, 64, 0.8, 1, qi(1), q(2), linetr_match_distmat_f64_workspace_bytes(5, 64) - 1, nullptr); }},
      {"tokenize/short", W, [&] { return linetr_tokenize(nullptr, recs, 3, 5, 8.0, 3, qf(11), qf(12), 2, 64, 96, 0, 0, 0, 0, tok, qi(13), q(14), linetr_tokenize_workspace_bytes(2, 64, 96, 5) - 1, nullptr); }},
      {"sample_descriptors/short", W, [&] { return linetr_sample_descriptors(nullptr, qf(0), 4, qf(1), 4, 8, 0, 0, qf(2), q(3), linetr_sample_descriptors_workspace_bytes(4, 8, 0) - 1, nullptr); }},
      {"point_descriptors/short", W, [&] { return linetr_point_descriptors(nullptr, qf(0), qi(1), 1, 4, qf(2), 4, 8, 0, 0, qf(3), q(4), linetr_point_descriptors_workspace_bytes(1, 4, 8, 0) - 1, nullptr); }},
      {"pool_distmat/short", W, [&] { return linetr_pool_distmat(nullptr, qf(0), 40, 50, qi(1), 30, qi(2), 35, qf(3), q(4), linetr_pool_distmat_workspace_bytes(30, 35) - 1, nullptr); }},
      {"pool_distmat_dense/short", W, [&] { return linetr_pool_distmat_dense(nullptr, qf(0), 40, 50, qf(1), 30, qf(2), 35, qf(3), q(4), linetr_pool_distmat_dense_workspace_bytes(30, 40, 35, 50) - 1, nullptr); }},
      // shapes out of range
      {"match_points/negative", A, [&] { return linetr_match_points(nullptr, qf(0), -1, qf(1), 31, 0.8f, 1, qf(2), qi(3), q(4), 1 << 20, nullptr); }},
      {"pair_tail/negative", A, [&] { return linetr_pair_tail(nullptr, qf(0), 33, qf(1), 31, 0.7f, qf(2), 40, qi(3), -30, qf(4), 50, qi(5), 35, 0.8f, 1, q(6), out_bytes, q(7), 1 << 20, nullptr); }},
      {"match_distmat/negative", A, [&] { return linetr_match_distmat(nullptr, qf(0), 17, -64, 0.8f, 1, qi(1), q(2), 1 << 20, nullptr); }},
      {"match_distmat_f64/negative", A, [&] { return linetr_match_distmat_f64(nullptr, (const double*)q(0), -5, 64, 0.8, 1, qi(1), q(2), 1 << 20, nullptr); }},
      {"pool_distmat/k_beyond_n", A, [&] { return linetr_pool_distmat(nullptr, qf(0), 40, 50, qi(1), 41, qi(2), 35, qf(3), q(4), 1 << 20, nullptr); }},
      {"pool_distmat_dense/k0_beyond_grid", A, [&] { return linetr_pool_distmat_dense(nullptr, qf(0), 40, 50, qf(1), 65536, qf(2), 35, qf(3), q(4), 1 << 20, nullptr); }},
      {"pool_distmat_dense/negative", A, [&] { return linetr_pool_distmat_dense(nullptr, qf(0), 40, -50, qf(1), 30, qf(2), 35, qf(3), q(4), 1 << 20, nullptr); }},
      {"sample_descriptors/no_cells", A, [&] { return linetr_sample_descriptors(nullptr, qf(0), 4, qf(1), 0, 8, 0, 0, qf(2), q(3), 1 << 20, nullptr); }},
      {"sample_descriptors/negative_n", A, [&] { return linetr_sample_descriptors(nullptr, qf(0), -4, qf(1), 4, 8, 0, 0, qf(2), q(3), 1 << 20, nullptr); }},
      {"point_descriptors/too_many", A, [&] { return linetr_point_descriptors(nullptr, qf(0), qi(1), 1, int64_t(1) << 31, qf(2), 4, 8, 0, 0, qf(3), q(4), 1 << 20, nullptr); }},
      {"tokenize/max_tokens", A, [&] { return linetr_tokenize(nullptr, recs, 3, 5, 8.0, 4097, qf(11), qf(12), 2, 64, 96, 0, 0, 0, 0, tok, qi(13), q(14), 1 << 24, nullptr); }},
      {"tokenize/height_not_8k", A, [&] { return linetr_tokenize(nullptr, recs, 3, 5, 8.0, 3, qf(11), qf(12), 2, 65, 96, 0, 0, 0, 0, tok, qi(13), q(14), 1 << 24, nullptr); }},
      {"superpoint_heads/no_cells", A, [&] { return linetr_superpoint_heads(nullptr, qf(0), qf(1), 1, 0, 8, qf(2), qf(3), qf(4), nullptr); }},
      {"superpoint_heads_rows/short_stride", A, [&] { return linetr_superpoint_heads_rows(nullptr, qf(0), 64, qf(1), 256, 1, 4, 8, qf(2), qf(3), qf(4), nullptr); }},
      {"superpoint_keypoints/no_rows", A, [&] { return linetr_superpoint_keypoints(nullptr, qf(0), 1, 0, 96, 4, 0.005f, 4, 1024, 400, qf(1), qf(2), qi(3), qi(4), q(5), 1 << 20, nullptr); }},
      {"superpoint_keypoints/pixels_beyond_int", A, [&] { return linetr_superpoint_keypoints(nullptr, qf(0), 1, 65536, 65536, 4, 0.005f, 4, 1024, 400, qf(1), qf(2), qi(3), qi(4), q(5), 1 << 20, nullptr); }},
      {"superpoint_keypoints/radius", A, [&] { return linetr_superpoint_keypoints(nullptr, qf(0), 1, 64, 96, -1, 0.005f, 4, 1024, 400, qf(1), qf(2), qi(3), qi(4), q(5), 1 << 20, nullptr); }},
      {"superpoint_keypoints/max_keypoints_0", A, [&] { return linetr_superpoint_keypoints(nullptr, qf(0), 1, 64, 96, 4, 0.005f, 4, 0, 400, qf(1), qf(2), qi(3), qi(4), q(5), 1 << 20, nullptr); }},
      {"sp_conv3x3/batch_0", A, [&] { return linetr_sp_conv3x3(nullptr, qf(0), 0, 16, 16, 64, qf(1), qf(2), 64, 0, qf(3), nullptr); }},
      {"sp_conv3x3/layer", A, [&] { return linetr_sp_conv3x3(nullptr, qf(0), 1, 16, 16, 63, qf(1), qf(2), 64, 0, qf(3), nullptr); }},
      {"sp_conv3x3/pool_2", A, [&] { return linetr_sp_conv3x3(nullptr, qf(0), 1, 16, 16, 64, qf(1), qf(2), 64, 2, qf(3), nullptr); }},
      {"sp_conv1a/width_0", A, [&] { return linetr_sp_conv1a(nullptr, qf(0), 1, 16, 0, qf(1), qf(2), qf(3), nullptr); }},
      {"sp_conv3x3_pack/layer", A, [&] { return linetr_sp_conv3x3_pack(qf(0), 64, 65, qf(1), nullptr); }},
      {"pack_slab/capacity", Cp, [&] { return linetr_pack_slab(qf(0), 100, qi(1), qi(2), 2, qi(3), 2, 99, 0, qf(4), nullptr); }},
      // null pointers
      {"pair_tail/null_output", Cp, [&] { return linetr_pair_tail(nullptr, qf(0), 33, qf(1), 31, 0.7f, qf(2), 40, qi(3), 30, qf(4), 50, qi(5), 35, 0.8f, 1, nullptr, out_bytes, q(7), 1 << 20, nullptr); }},
      {"pair_tail/null_workspace", W, [&] { return linetr_pair_tail(nullptr, qf(0), 33, qf(1), 31, 0.7f, qf(2), 40, qi(3), 30, qf(4), 50, qi(5), 35, 0.8f, 1, q(6), out_bytes, nullptr, 1 << 20, nullptr); }},
      {"match_distmat/null_output", A, [&] { return linetr_match_distmat(nullptr, qf(0), 17, 64, 0.8f, 1, nullptr, q(2), 1 << 20, nullptr); }},
      {"match_distmat_f64/null_matrix", A, [&] { return linetr_match_distmat_f64(nullptr, nullptr, 5, 64, 0.8, 1, qi(1), q(2), 1 << 20, nullptr); }},
      {"pool_distmat/null_map", A, [&] { return linetr_pool_distmat(nullptr, qf(0), 40, 50, nullptr, 30, qi(2), 35, qf(3), q(4), 1 << 20, nullptr); }},
      {"pool_distmat_dense/null_output", A, [&] { return linetr_pool_distmat_dense(nullptr, qf(0), 40, 50, qf(1), 30, qf(2), 35, nullptr, q(4), 1 << 20, nullptr); }},
      {"sample_descriptors/null_points", A, [&] { return linetr_sample_descriptors(nullptr, nullptr, 4, qf(1), 4, 8, 0, 0, qf(2), q(3), 1 << 20, nullptr); }},
      {"point_descriptors/null_offsets", A, [&] { return linetr_point_descriptors(nullptr, qf(0), nullptr, 1, 4, qf(2), 4, 8, 0, 0, qf(3), q(4), 1 << 20, nullptr); }},
      {"tokenize/null_records", A, [&] { return linetr_tokenize(nullptr, nullptr, 3, 5, 8.0, 3, qf(11), qf(12), 2, 64, 96, 0, 0, 0, 0, tok, qi(13), q(14), 1 << 24, nullptr); }},
      {"superpoint_heads/score_without_logits", A, [&] { return linetr_superpoint_heads(nullptr, nullptr, qf(1), 1, 4, 8, qf(2), qf(3), qf(4), nullptr); }},
      {"sp_conv3x3/null_input", A, [&] { return linetr_sp_conv3x3(nullptr, nullptr, 1, 16, 16, 64, qf(1), qf(2), 64, 0, qf(3), nullptr); }},
      {"sp_conv1a/null_bias", A, [&] { return linetr_sp_conv1a(nullptr, qf(0), 1, 16, 16, qf(1), nullptr, qf(3), nullptr); }},
      {"sp_conv3x3_pack/null_output", A, [&] { return linetr_sp_conv3x3_pack(qf(0), 64, 64, nullptr, nullptr); }},
      {"sp_encoder_create/null_output", A, [&] { return linetr_sp_encoder_create(0, nullptr); }},
      {"sp_encoder_set_weights/null_encoder", A, [&] { return linetr_sp_encoder_set_weights(nullptr, nullptr, nullptr, nullptr); }},
      {"sp_encoder_forward/null_encoder", A, [&] { return linetr_sp_encoder_forward(nullptr, qf(0), 1, 64, 96, qf(1), qf(2), nullptr, q(3), 1 << 20, nullptr); }},
      {"pack_slab/null_slab", A, [&] { return linetr_pack_slab(qf(0), 10, qi(1), qi(2), 2, qi(3), 2, 99, 0, nullptr, nullptr); }},
      {"set_profiling/null_handle", A, [&] { return linetr_set_profiling(nullptr, 1); }},
      {"get_profile/null_handle", A, [&] { return linetr_get_profile(nullptr, nullptr, 0, nullptr); }},
      {"allgather_desc/null_communicator", A, [&] { return linetr_allgather_desc(nullptr, q(0), q(1), 256, nullptr); }},
      // misaligned pointers
      {"sample_descriptors/misaligned_output", A, [&] { return linetr_sample_descriptors(nullptr, qf(0), 4, qf(1), 4, 8, 0, 0, odd(2), q(3), 1 << 20, nullptr); }},
      {"point_descriptors/misaligned_workspace", A, [&] { return linetr_point_descriptors(nullptr, qf(0), qi(1), 1, 4, qf(2), 4, 8, 0, 0, qf(3), odd(4), 1 << 20, nullptr); }},
      {"tokenize/misaligned_workspace", A, [&] { return linetr_tokenize(nullptr, recs, 3, 5, 8.0, 3, qf(11), qf(12), 2, 64, 96, 0, 0, 0, 0, tok, qi(13), odd(14), 1 << 24, nullptr); }},
      {"superpoint_heads/misaligned_map", A, [&] { return linetr_superpoint_heads(nullptr, qf(0), qf(1), 1, 4, 8, odd(2), qf(3), qf(4), nullptr); }},
      {"sp_conv3x3/misaligned_output", A, [&] { return linetr_sp_conv3x3(nullptr, qf(0), 1, 16, 16, 64, qf(1), qf(2), 64, 0, odd(3), nullptr); }},
      {"sp_conv1a/misaligned_image", A, [&] { return linetr_sp_conv1a(nullptr, odd(0), 1, 16, 16, qf(1), qf(2), qf(3), nullptr); }},
  };
  run_refusals(t, "refusals_out.txt");
  CHECK(linetr_set_precision(nullptr, 1) == LINETR_E_ARG && !strcmp(last_error(), STALE), "linetr_set_precision(NULL) is not refused");
  CHECK(linetr_get_precision(nullptr) == LINETR_E_ARG, "linetr_get_precision(NULL) is not LINETR_E_ARG");
  CHECK(block.all_bytes(0), "a refused call wrote into the block its pointers came from");
  return 0;
}

// The entry points of the photometric, view, detector and training units: every refusal of theirs is decided before the first launch
// (their bodies say so), and these are the ones that read caller HOST tables -- the parameter records, kernel sizes and sigmas,
// homography matrices, the optimizer's tensor table, the prefix sums and pseudo records of the fixed-size samples, the configuration
// structs.  Each table is a heap allocation of exactly the documented size; the planted bad entry is the LAST one, so the refusal is
// reached only after the whole table has been read.
int cmd_refusals_tables() {
  Heap<unsigned char> block(16384 + 256);
  const uintptr_t p0 = ((uintptr_t)block.p + 255) / 256 * 256;
  auto q = [&](int i) { return (void*)(p0 + 256 * (uintptr_t)i); };
  auto qf = [&](int i) { return (float*)q(i); };
  auto qi = [&](int i) { return (int32_t*)q(i); };
  auto off = [&](int i, int bytes) { return (float*)(p0 + 256 * (uintptr_t)i + bytes); };
  const double NaN = std::numeric_limits<double>::quiet_NaN();
  const int A = LINETR_E_ARG, W = LINETR_E_WORKSPACE;
  const int64_t BIG = int64_t(1) << 40;

  // ---- photometric: h_params [B] of 1224-byte records
  const int B = 5, H = 8, Wd = 12;
  auto good_params = [&] {
    Heap<LinetrPhotoParams> t((size_t)B);
    for (int b = 0; b < B; ++b) { t.p[b].alpha = 1.0; t.p[b].K = 1; t.p[b].weights[0] = 1.f; t.p[b].blur_ksize = 1; t.p[b].shade_ksize = 1; }
    return t;
  };
  const Heap<LinetrPhotoParams> good = good_params();
  const int64_t photo_need = linetr_photometric_workspace_bytes(B, 1, H, Wd);
  auto photo = [&](const LinetrPhotoParams* params, int b, int h, int w, uint64_t seed, int first, int quant, const float* src, float* dst, void* ws, int64_t ws_bytes) {
    return linetr_photometric(nullptr, src, b, h, w, params, seed, first, quant, dst, ws, ws_bytes, nullptr);
  };
  auto planted = [&](std::function<void(LinetrPhotoParams&)> f) {
    Heap<LinetrPhotoParams> t = good_params();
    f(t.p[B - 1]);
    return photo(t.p, B, H, Wd, 1, 0, 0, qf(0), qf(8), q(16), BIG);
  };
  // ---- gaussian blur: h_ksize [B], h_sigma [B]
  auto blur = [&](int last_ksize, double last_sigma, int b, int c, const float* src, float* dst, void* ws, int64_t ws_bytes, int quant = 0) {
    Heap<int32_t> ks((size_t)B); Heap<double> sg((size_t)B);
    for (int i = 0; i < B; ++i) { ks.p[i] = 3; sg.p[i] = 0.0; }
    ks.p[B - 1] = last_ksize; sg.p[B - 1] = last_sigma;
    return linetr_gaussian_blur(nullptr, src, b, c, H, Wd, ks.p, sg.p, quant, dst, ws, ws_bytes, nullptr);
  };
  // ---- warp: h_mat [B][9]
  auto warp = [&](double last, int b, int c, int h, int w, int mode, const float* src, float* dst) {
    Heap<double> m((size_t)B * 9);
    for (int i = 0; i < B; ++i) m.p[9 * i] = m.p[9 * i + 4] = m.p[9 * i + 8] = 1.0;
    m.p[B * 9 - 1] = last;
    return linetr_warp_images(nullptr, src, b, c, h, w, m.p, mode, dst, nullptr, nullptr);
  };
  // ---- detector: the configuration struct
  auto detect = [&](std::function<void(LinetrDetectConfig&)> f, int b, int h, int w, int is_float, int cap, const void* img, double* rows, int32_t* counts, void* ws,
                    int64_t ws_bytes) {
    Heap<LinetrDetectConfig> c(1);
    c.p->n_octaves = 2; c.p->scale = 2; c.p->grad_threshold = 28160; c.p->min_region_size = 16; c.p->density = 0.6;
    f(*c.p);
    return linetr_detect_lines(nullptr, img, is_float, b, h, w, c.p, cap, rows, counts, nullptr, ws, ws_bytes, nullptr);
  };
  auto same = [](LinetrDetectConfig&) {};
  Heap<int32_t> det_counts(2);
  const int64_t det_need = linetr_detect_lines_workspace_bytes(2, 64, 96, 2);
  // ---- optimizer: LinetrAdamTensor h_table [n], LinetrAdamHyper
  const int NT = 6;
  auto adam_table = [&] {
    Heap<LinetrAdamTensor> t((size_t)NT);
    for (int i = 0; i < NT; ++i) {
      t.p[i].p = qf(4 * i); t.p[i].g = qf(4 * i + 1); t.p[i].m = qf(4 * i + 2); t.p[i].v = qf(4 * i + 3);
      t.p[i].n = 10; t.p[i].step_size = 1e-3f; t.p[i].bc2_sqrt = 0.5f;
    }
    return t;
  };
  auto adam = [&](std::function<void(LinetrAdamTensor&)> ft, std::function<void(LinetrAdamHyper&)> fh, int n, void* ws, int64_t ws_bytes, const float* scale = nullptr) {
    Heap<LinetrAdamTensor> t = adam_table();
    ft(t.p[NT - 1]);
    Heap<LinetrAdamHyper> hy(1);
    hy.p->beta1 = 0.9; hy.p->beta2 = 0.999; hy.p->eps = 1e-8; hy.p->weight_decay = 0.0; hy.p->lr = 1e-3; hy.p->decoupled = 0;
    fh(*hy.p);
    return linetr_adam_step(nullptr, t.p, n, hy.p, scale, ws, ws_bytes, nullptr);
  };
  auto norm = [&](std::function<void(LinetrAdamTensor&)> ft, int n, double max_norm, double* d_norm, float* d_scale, void* ws, int64_t ws_bytes) {
    Heap<LinetrAdamTensor> t = adam_table();
    ft(t.p[NT - 1]);
    return linetr_grad_norm(nullptr, t.p, n, max_norm, d_norm, d_scale, ws, ws_bytes, nullptr);
  };
  auto keep_t = [](LinetrAdamTensor&) {};
  auto keep_h = [](LinetrAdamHyper&) {};
  const int64_t adam_need = linetr_adam_workspace_bytes(NT, 60), norm_need = linetr_grad_norm_workspace_bytes(NT, 60);
  // ---- fixed-size samples: h_cu_k / h_cu_n / h_cu_p [B + 1], h_pseudo [h_cu_p[B]]
  const int FB = 3, M = 4, T = 21;
  LinetrTokens tok{};
  tok.klines = qf(0); tok.length = qf(1); tok.angles = qf(2); tok.sublines = qf(3); tok.pnt = qf(4); tok.mask = qf(5); tok.resp = qf(6);
  tok.angle_sub = qf(7); tok.desc = qf(8); tok.score = qf(9); tok.mat = qf(10);
  const int64_t fs_need = linetr_fixed_size_workspace_bytes(FB, 64, 96, 0);
  // per image: 2 key-lines, 3 sub-lines, so M - 3 = 1 pseudo line each
  auto fixed = [&](std::function<void(int32_t*, int32_t*, int32_t*, LinetrLineRec*)> f, int b, int m, int t, double td, int height, const float* desc,
                   void* ws, int64_t ws_bytes, bool with_pseudo = true) {
    Heap<int32_t> ck((size_t)FB + 1), cn((size_t)FB + 1), cp((size_t)FB + 1);
    for (int i = 0; i <= FB; ++i) { ck.p[i] = 2 * i; cn.p[i] = 3 * i; cp.p[i] = i; }
    Heap<LinetrLineRec> ps((size_t)FB);
    for (int i = 0; i < FB; ++i) { ps.p[i].n_sub = 1; ps.p[i].n_tok = 5; ps.p[i].image = i; ps.p[i].line_local = 0; }
    f(ck.p, cn.p, cp.p, ps.p);
    return linetr_fixed_size(nullptr, (const LinetrLineRec*)q(11), ck.p, cn.p, (const LinetrLineRec*)q(12), with_pseudo ? ps.p : nullptr, cp.p, b, m, t, td, desc,
                             qf(14), height, 96, 0, 0, 0, 0, 0, 0, tok, qi(15), qi(16), ws, ws_bytes, nullptr);
  };
  auto keep_fs = [](int32_t*, int32_t*, int32_t*, LinetrLineRec*) {};
  // ---- the criterion, ground truth and the backward passes: device pointers only, sizes from their queries
  Heap<int64_t> val_offs(4);
  const int64_t val_out = linetr_val_step_output_bytes(2, val_offs.p), val_ws = linetr_val_step_workspace_bytes(2, 64);
  const int64_t lg_ws = linetr_desc_loss_grad_workspace_bytes(2, 64);
  auto val = [&](int n0, int n1, int b, const float* d0, void* pinned, int64_t pinned_bytes, void* ws, int64_t ws_bytes) {
    return linetr_val_step(nullptr, d0, n0, qf(1), n1, qf(2), b, 0.8, 1, nullptr, nullptr, nullptr, pinned, pinned_bytes, ws, ws_bytes, nullptr);
  };
  auto lossgrad = [&](int n0, int n1, int b, const float* d0, void* pinned, int64_t pinned_bytes, void* ws, int64_t ws_bytes) {
    return linetr_desc_loss_grad(nullptr, d0, n0, qf(1), n1, qf(2), b, nullptr, qf(3), qf(4), pinned, pinned_bytes, ws, ws_bytes, nullptr);
  };
  auto gt = [&](int coord, int n0, int n1, int b, int pad, int m, const void* l0, const double* hm, void* ws, int64_t ws_bytes) {
    return linetr_gt_assign(nullptr, coord, l0, n0, q(1), n1, hm, b, nullptr, nullptr, 5.0, 5.0, 0.2, pad, qf(3), qi(4), m, qi(5), nullptr, nullptr, nullptr, nullptr, ws,
                            ws_bytes, nullptr);
  };
  const int64_t gt_need = linetr_gt_assign_workspace_bytes(2, 64, 64);
  auto linbwd = [&](int64_t rows, int n, int k, int64_t ldx, const float* x, float* dw, void* ws, int64_t ws_bytes) {
    return linetr_linear_backward(nullptr, x, ldx, qf(1), qf(2), n, nullptr, rows, n, k, qf(3), dw, qf(5), ws, ws_bytes, nullptr);
  };
  auto bnf = [&](int64_t rows, int c, int mode, float eps, const float* z, float* running, void* ws, int64_t ws_bytes) {
    return linetr_bn_forward(nullptr, z, c, rows, c, qf(1), qf(2), eps, 0.1f, running, mode, 1, qf(4), c, (double*)q(5), ws, ws_bytes, nullptr);
  };
  auto bnb = [&](int64_t rows, int c, int mode, int64_t ldz, const float* z, void* ws, int64_t ws_bytes) {
    return linetr_bn_backward(nullptr, z, ldz, nullptr, 0, qf(1), c, (const double*)q(2), qf(3), rows, c, mode, qf(4), c, qf(5), qf(6), ws, ws_bytes, nullptr);
  };
  auto lnb = [&](int64_t rows, int c, int64_t lda, const float* a, void* ws, int64_t ws_bytes) {
    return linetr_layer_norm_backward(nullptr, a, lda, nullptr, 0, qf(1), qf(2), qf(3), 256, rows, c, qf(4), 256, qf(5), qf(6), ws, ws_bytes, nullptr);
  };
  auto headb = [&](int64_t rows, const float* x, const float* bias, void* ws, int64_t ws_bytes) {
    return linetr_head_backward(nullptr, x, qf(1), bias, qf(3), rows, qf(4), qf(5), qf(6), ws, ws_bytes, nullptr);
  };
  auto inb = [&](int64_t rows, int n, int kin, const float* x, void* ws, int64_t ws_bytes) {
    return linetr_input_layer_backward(nullptr, x, kin, qf(1), n, rows, n, kin, qf(2), qf(3), ws, ws_bytes, nullptr);
  };
  auto tab = [&](int64_t l, int s, const float* dx, void* ws, int64_t ws_bytes) {
    return linetr_token_assemble_backward(nullptr, dx, l, s, qf(1), qf(2), ws, ws_bytes, nullptr);
  };
  auto labels = [&](int b, int h, int w, const int8_t* buckets, int32_t* lab, void* ws, int64_t ws_bytes) {
    return linetr_detect_debug_labels(nullptr, buckets, b, h, w, lab, ws, ws_bytes, nullptr);
  };
  auto erode = [&](int b, int h, int w, int radius, const uint8_t* mask, uint8_t* out) { return linetr_mask_erode(nullptr, mask, b, h, w, radius, out, nullptr); };

  // ---- the dropout state: one exact-size LinetrDropout
  auto dropout = [&](std::function<void(LinetrDropout&)> f, std::function<int(const LinetrDropout*)> call) {
    Heap<LinetrDropout> d(1);
    d.p->seed = 2026; d.p->call = 1; d.p->threshold = 429496730u; d.p->scale = 1.f / 0.9f;
    f(*d.p);
    return call(d.p);
  };

  std::vector<Refusal> t = {
      // linetr_photometric
      {"photometric/short", W, [&] { return photo(good.p, B, H, Wd, 1, 0, 0, qf(0), qf(8), q(16), photo_need - 1); }},
      {"photometric/null_params", A, [&] { return photo(nullptr, B, H, Wd, 1, 0, 0, qf(0), qf(8), q(16), BIG); }},
      {"photometric/null_source", A, [&] { return photo(good.p, B, H, Wd, 1, 0, 0, nullptr, qf(8), q(16), BIG); }},
      {"photometric/null_workspace", A, [&] { return photo(good.p, B, H, Wd, 1, 0, 0, qf(0), qf(8), nullptr, BIG); }},
      {"photometric/batch_0", A, [&] { return photo(good.p, 0, H, Wd, 1, 0, 0, qf(0), qf(8), q(16), BIG); }},
      {"photometric/height_beyond", A, [&] { return photo(good.p, B, 32769, Wd, 1, 0, 0, qf(0), qf(8), q(16), BIG); }},
      {"photometric/seed_beyond_32_bits", A, [&] { return photo(good.p, B, H, Wd, uint64_t(1) << 32, 0, 0, qf(0), qf(8), q(16), BIG); }},
      {"photometric/first_negative", A, [&] { return photo(good.p, B, H, Wd, 1, -1, 0, qf(0), qf(8), q(16), BIG); }},
      {"photometric/first_beyond", A, [&] { return photo(good.p, B, H, Wd, 1, INT32_MAX - 1, 0, qf(0), qf(8), q(16), BIG); }},
      {"photometric/quantise_2", A, [&] { return photo(good.p, B, H, Wd, 1, 0, 2, qf(0), qf(8), q(16), BIG); }},
      {"photometric/in_place", A, [&] { return photo(good.p, B, H, Wd, 1, 0, 0, qf(0), qf(0), q(16), BIG); }},
      {"photometric/misaligned_source", A, [&] { return photo(good.p, B, H, Wd, 1, 0, 0, off(0, 2), qf(8), q(16), BIG); }},
      {"photometric/misaligned_workspace", A, [&] { return photo(good.p, B, H, Wd, 1, 0, 0, qf(0), qf(8), off(16, 16), BIG); }},
      {"photometric/last_record_stage_bits", A, [&] { return planted([](LinetrPhotoParams& p) { p.stages = 128; }); }},
      {"photometric/last_record_d", A, [&] { return planted([](LinetrPhotoParams& p) { p.d = 256; }); }},
      {"photometric/last_record_alpha_nan", A, [&] { return planted([&](LinetrPhotoParams& p) { p.alpha = NaN; }); }},
      {"photometric/last_record_sigma_negative", A, [&] { return planted([](LinetrPhotoParams& p) { p.sigma = -1.0; }); }},
      {"photometric/last_record_K_2", A, [&] { return planted([](LinetrPhotoParams& p) { p.K = 2; }); }},
      {"photometric/last_record_last_weight_nan", A, [&] { return planted([&](LinetrPhotoParams& p) { p.weights[48] = (float)NaN; }); }},
      {"photometric/last_record_blur_ksize_even", A, [&] { return planted([](LinetrPhotoParams& p) { p.blur_ksize = 4; }); }},
      {"photometric/last_record_shade_ksize_353", A, [&] { return planted([](LinetrPhotoParams& p) { p.shade_ksize = 353; }); }},
      {"photometric/last_record_ellipses_21", A, [&] { return planted([](LinetrPhotoParams& p) { p.n_ellipses = 21; }); }},
      {"photometric/last_record_last_ellipse_axis_0", A, [&] { return planted([](LinetrPhotoParams& p) {
         p.n_ellipses = 20;
         for (int e = 0; e < 20; ++e) { double v[6] = {3, 3, 2, 2, 1, 0}; memcpy(p.ellipse[e], v, sizeof v); }
         p.ellipse[19][3] = 0.0; }); }},
      {"photometric/last_record_last_ellipse_nan", A, [&] { return planted([&](LinetrPhotoParams& p) {
         p.n_ellipses = 20;
         for (int e = 0; e < 20; ++e) { double v[6] = {3, 3, 2, 2, 1, 0}; memcpy(p.ellipse[e], v, sizeof v); }
         p.ellipse[19][5] = NaN; }); }},
      // linetr_gaussian_blur
      {"gaussian_blur/short", W, [&] { return blur(3, 0.0, B, 1, qf(0), qf(8), q(16), photo_need - 1); }},
      {"gaussian_blur/last_ksize_even", A, [&] { return blur(4, 0.0, B, 1, qf(0), qf(8), q(16), BIG); }},
      {"gaussian_blur/last_ksize_353", A, [&] { return blur(353, 0.0, B, 1, qf(0), qf(8), q(16), BIG); }},
      {"gaussian_blur/last_sigma_negative", A, [&] { return blur(3, -1.0, B, 1, qf(0), qf(8), q(16), BIG); }},
      {"gaussian_blur/last_sigma_nan", A, [&] { return blur(3, NaN, B, 1, qf(0), qf(8), q(16), BIG); }},
      {"gaussian_blur/channels_0", A, [&] { return blur(3, 0.0, B, 0, qf(0), qf(8), q(16), BIG); }},
      {"gaussian_blur/quantise_2", A, [&] { return blur(3, 0.0, B, 1, qf(0), qf(8), q(16), BIG, 2); }},
      {"gaussian_blur/null_destination", A, [&] { return blur(3, 0.0, B, 1, qf(0), nullptr, q(16), BIG); }},
      {"gaussian_blur/misaligned_destination", A, [&] { return blur(3, 0.0, B, 1, qf(0), off(8, 2), q(16), BIG); }},
      {"gaussian_blur/null_ksize", A, [&] { Heap<double> sg((size_t)B); return linetr_gaussian_blur(nullptr, qf(0), B, 1, H, Wd, nullptr, sg.p, 0, qf(8), q(16), BIG, nullptr); }},
      {"gaussian_blur/null_sigma", A, [&] { Heap<int32_t> ks((size_t)B); return linetr_gaussian_blur(nullptr, qf(0), B, 1, H, Wd, ks.p, nullptr, 0, qf(8), q(16), BIG, nullptr); }},
      // linetr_warp_images, linetr_mask_erode
      {"warp_images/last_matrix_entry_nan", A, [&] { return warp(NaN, B, 1, H, Wd, 0, qf(0), qf(8)); }},
      {"warp_images/null_matrices", A, [&] { return linetr_warp_images(nullptr, qf(0), B, 1, H, Wd, nullptr, 0, qf(8), nullptr, nullptr); }},
      {"warp_images/mode_2", A, [&] { return warp(1.0, B, 1, H, Wd, 2, qf(0), qf(8)); }},
      {"warp_images/batch_0", A, [&] { return warp(1.0, 0, 1, H, Wd, 0, qf(0), qf(8)); }},
      {"warp_images/elements_beyond_int", A, [&] { return warp(1.0, B, 4, 32768, 32768, 0, qf(0), qf(8)); }},
      {"warp_images/in_place", A, [&] { return warp(1.0, B, 1, H, Wd, 0, qf(0), qf(0)); }},
      {"warp_images/misaligned_source", A, [&] { return warp(1.0, B, 1, H, Wd, 0, off(0, 2), qf(8)); }},
      {"warp_images/null_destination", A, [&] { return warp(1.0, B, 1, H, Wd, 0, qf(0), nullptr); }},
      {"mask_erode/radius_negative", A, [&] { return erode(2, 8, 8, -1, (const uint8_t*)q(0), (uint8_t*)q(8)); }},
      {"mask_erode/overlapping", A, [&] { return erode(2, 8, 8, 2, (const uint8_t*)q(0), (uint8_t*)q(0) + 64); }},
      {"mask_erode/null_mask", A, [&] { return erode(2, 8, 8, 2, nullptr, (uint8_t*)q(8)); }},
      {"mask_erode/width_0", A, [&] { return erode(2, 8, 0, 2, (const uint8_t*)q(0), (uint8_t*)q(8)); }},
      // linetr_detect_lines, linetr_detect_debug_labels (their short workspace is LINETR_E_ARG)
      {"detect_lines/short", A, [&] { return detect(same, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), det_need - 1); }},
      {"detect_lines/null_config", A, [&] { return linetr_detect_lines(nullptr, q(0), 0, 2, 64, 96, nullptr, 100, (double*)q(1), det_counts.p, nullptr, q(2), BIG, nullptr); }},
      {"detect_lines/octaves_13", A, [&] { return detect([](LinetrDetectConfig& c) { c.n_octaves = 13; }, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/scale_3", A, [&] { return detect([](LinetrDetectConfig& c) { c.scale = 3; }, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/threshold_0", A, [&] { return detect([](LinetrDetectConfig& c) { c.grad_threshold = 0; }, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/region_size_3", A, [&] { return detect([](LinetrDetectConfig& c) { c.min_region_size = 3; }, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/density_nan", A, [&] { return detect([&](LinetrDetectConfig& c) { c.density = NaN; }, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/batch_0", A, [&] { return detect(same, 0, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/null_counts", A, [&] { return detect(same, 2, 64, 96, 0, 100, q(0), (double*)q(1), nullptr, q(2), BIG); }},
      {"detect_lines/images_are_float_2", A, [&] { return detect(same, 2, 64, 96, 2, 100, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/capacity_negative", A, [&] { return detect(same, 2, 64, 96, 0, -1, q(0), (double*)q(1), det_counts.p, q(2), BIG); }},
      {"detect_lines/misaligned_rows", A, [&] { return detect(same, 2, 64, 96, 0, 100, q(0), (double*)off(1, 4), det_counts.p, q(2), BIG); }},
      {"detect_lines/misaligned_workspace", A, [&] { return detect(same, 2, 64, 96, 0, 100, q(0), (double*)q(1), det_counts.p, off(2, 128), BIG); }},
      {"detect_debug_labels/short", A, [&] { return labels(2, 8, 12, (const int8_t*)q(0), qi(1), q(2), 2 * 8 * 12 * 4 - 1); }},
      {"detect_debug_labels/batch_0", A, [&] { return labels(0, 8, 12, (const int8_t*)q(0), qi(1), q(2), BIG); }},
      {"detect_debug_labels/null_buckets", A, [&] { return labels(2, 8, 12, nullptr, qi(1), q(2), BIG); }},
      {"detect_debug_labels/misaligned_labels", A, [&] { return labels(2, 8, 12, (const int8_t*)q(0), (int32_t*)off(1, 2), q(2), BIG); }},
      // linetr_adam_step, linetr_grad_norm (a short workspace is LINETR_E_ARG there)
      {"adam_step/short", A, [&] { return adam(keep_t, keep_h, NT, q(40), adam_need - 1); }},
      {"adam_step/null_table", A, [&] { Heap<LinetrAdamHyper> hy(1); return linetr_adam_step(nullptr, nullptr, NT, hy.p, nullptr, q(40), BIG, nullptr); }},
      {"adam_step/no_tensors", A, [&] { return adam(keep_t, keep_h, 0, q(40), BIG); }},
      {"adam_step/last_entry_n_negative", A, [&] { return adam([](LinetrAdamTensor& e) { e.n = -1; }, keep_h, NT, q(40), BIG); }},
      {"adam_step/last_entry_null_v", A, [&] { return adam([](LinetrAdamTensor& e) { e.v = nullptr; }, keep_h, NT, q(40), BIG); }},
      {"adam_step/last_entry_misaligned_g", A, [&] { return adam([&](LinetrAdamTensor& e) { e.g = off(30, 2); }, keep_h, NT, q(40), BIG); }},
      {"adam_step/last_entry_equal_pointers", A, [&] { return adam([](LinetrAdamTensor& e) { e.m = e.p; }, keep_h, NT, q(40), BIG); }},
      {"adam_step/last_entry_step_size_nan", A, [&] { return adam([&](LinetrAdamTensor& e) { e.step_size = (float)NaN; }, keep_h, NT, q(40), BIG); }},
      {"adam_step/last_entry_bc2_sqrt_0", A, [&] { return adam([](LinetrAdamTensor& e) { e.bc2_sqrt = 0.f; }, keep_h, NT, q(40), BIG); }},
      {"adam_step/null_hyper", A, [&] { Heap<LinetrAdamTensor> tt = adam_table(); return linetr_adam_step(nullptr, tt.p, NT, nullptr, nullptr, q(40), BIG, nullptr); }},
      {"adam_step/beta1_1", A, [&] { return adam(keep_t, [](LinetrAdamHyper& y) { y.beta1 = 1.0; }, NT, q(40), BIG); }},
      {"adam_step/eps_nan", A, [&] { return adam(keep_t, [&](LinetrAdamHyper& y) { y.eps = NaN; }, NT, q(40), BIG); }},
      {"adam_step/decoupled_2", A, [&] { return adam(keep_t, [](LinetrAdamHyper& y) { y.decoupled = 2; }, NT, q(40), BIG); }},
      {"adam_step/decoupled_lr_nan", A, [&] { return adam(keep_t, [&](LinetrAdamHyper& y) { y.decoupled = 1; y.lr = NaN; }, NT, q(40), BIG); }},
      {"adam_step/misaligned_grad_scale", A, [&] { return adam(keep_t, keep_h, NT, q(40), BIG, off(39, 2)); }},
      {"adam_step/misaligned_workspace", A, [&] { return adam(keep_t, keep_h, NT, off(40, 16), BIG); }},
      {"adam_step/null_workspace", A, [&] { return adam(keep_t, keep_h, NT, nullptr, BIG); }},
      {"grad_norm/short", A, [&] { return norm(keep_t, NT, 1.0, (double*)q(38), qf(39), q(40), norm_need - 1); }},
      {"grad_norm/last_entry_null_g", A, [&] { return norm([](LinetrAdamTensor& e) { e.g = nullptr; }, NT, 1.0, (double*)q(38), qf(39), q(40), BIG); }},
      {"grad_norm/last_entry_n_negative", A, [&] { return norm([](LinetrAdamTensor& e) { e.n = INT64_MIN; }, NT, 1.0, (double*)q(38), qf(39), q(40), BIG); }},
      {"grad_norm/max_norm_negative", A, [&] { return norm(keep_t, NT, -1.0, (double*)q(38), qf(39), q(40), BIG); }},
      {"grad_norm/max_norm_nan", A, [&] { return norm(keep_t, NT, NaN, (double*)q(38), qf(39), q(40), BIG); }},
      {"grad_norm/null_norm", A, [&] { return norm(keep_t, NT, 1.0, nullptr, qf(39), q(40), BIG); }},
      {"grad_norm/misaligned_norm", A, [&] { return norm(keep_t, NT, 1.0, (double*)off(38, 4), qf(39), q(40), BIG); }},
      // linetr_fixed_size
      {"fixed_size/short", W, [&] { return fixed(keep_fs, FB, M, T, 8.0, 64, qf(13), q(17), fs_need - 1); }},
      {"fixed_size/batch_0", A, [&] { return fixed(keep_fs, 0, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/height_not_8k", A, [&] { return fixed(keep_fs, FB, M, T, 8.0, 65, qf(13), q(17), BIG); }},
      {"fixed_size/max_sublines_0", A, [&] { return fixed(keep_fs, FB, 0, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/max_tokens_4097", A, [&] { return fixed(keep_fs, FB, M, 4097, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/token_distance_nan", A, [&] { return fixed(keep_fs, FB, M, T, NaN, 64, qf(13), q(17), BIG); }},
      {"fixed_size/null_descriptors", A, [&] { return fixed(keep_fs, FB, M, T, 8.0, 64, nullptr, q(17), BIG); }},
      {"fixed_size/null_workspace", A, [&] { return fixed(keep_fs, FB, M, T, 8.0, 64, qf(13), nullptr, BIG); }},
      {"fixed_size/prefix_not_from_0", A, [&] { return fixed([](int32_t* k, int32_t*, int32_t*, LinetrLineRec*) { k[0] = 1; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/last_prefix_descends", A, [&] { return fixed([&](int32_t* k, int32_t*, int32_t*, LinetrLineRec*) { k[FB] = k[FB - 1] - 1; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/last_image_fewer_sublines_than_lines", A, [&] { return fixed([&](int32_t*, int32_t* n, int32_t*, LinetrLineRec*) { n[FB] = n[FB - 1] + 1; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/last_image_too_many_lines", A, [&] { return fixed([&](int32_t* k, int32_t* n, int32_t*, LinetrLineRec*) { k[FB] = k[FB - 1] + M + 1; n[FB] = n[FB - 1] + M + 1; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/last_image_pseudo_count", A, [&] { return fixed([&](int32_t*, int32_t*, int32_t* p, LinetrLineRec*) { p[FB] = p[FB - 1]; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/null_pseudo_records", A, [&] { return fixed(keep_fs, FB, M, T, 8.0, 64, qf(13), q(17), BIG, false); }},
      {"fixed_size/last_pseudo_two_sublines", A, [&] { return fixed([&](int32_t*, int32_t*, int32_t*, LinetrLineRec* r) { r[FB - 1].n_sub = 2; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/last_pseudo_too_many_tokens", A, [&] { return fixed([&](int32_t*, int32_t*, int32_t*, LinetrLineRec* r) { r[FB - 1].n_tok = T + 1; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/last_pseudo_wrong_image", A, [&] { return fixed([&](int32_t*, int32_t*, int32_t*, LinetrLineRec* r) { r[FB - 1].image = 0; }, FB, M, T, 8.0, 64, qf(13), q(17), BIG); }},
      {"fixed_size/misaligned_workspace", A, [&] { return fixed(keep_fs, FB, M, T, 8.0, 64, qf(13), off(17, 4), BIG); }},
      // linetr_val_step, linetr_desc_loss_grad, linetr_gt_assign (short blocks are LINETR_E_ARG there)
      {"val_step/short", A, [&] { return val(64, 64, 2, qf(0), q(6), val_out, q(7), val_ws - 1); }},
      {"val_step/output_short", A, [&] { return val(64, 64, 2, qf(0), q(6), val_out - 1, q(7), BIG); }},
      {"val_step/sides_differ", A, [&] { return val(64, 63, 2, qf(0), q(6), BIG, q(7), BIG); }},
      {"val_step/batch_0", A, [&] { return val(64, 64, 0, qf(0), q(6), BIG, q(7), BIG); }},
      {"val_step/n_beyond", A, [&] { return val(32769, 32769, 2, qf(0), q(6), BIG, q(7), BIG); }},
      {"val_step/null_descriptors", A, [&] { return val(64, 64, 2, nullptr, q(6), BIG, q(7), BIG); }},
      {"val_step/null_output", A, [&] { return val(64, 64, 2, qf(0), nullptr, BIG, q(7), BIG); }},
      {"desc_loss_grad/short", A, [&] { return lossgrad(64, 64, 2, qf(0), q(6), BIG, q(7), lg_ws - 1); }},
      {"desc_loss_grad/output_short", A, [&] { return lossgrad(64, 64, 2, qf(0), q(6), 8, q(7), BIG); }},
      {"desc_loss_grad/sides_differ", A, [&] { return lossgrad(63, 64, 2, qf(0), q(6), BIG, q(7), BIG); }},
      {"desc_loss_grad/null_workspace", A, [&] { return lossgrad(64, 64, 2, qf(0), q(6), BIG, nullptr, BIG); }},
      {"gt_assign/short", A, [&] { return gt(0, 64, 64, 2, 1, 10, q(0), (const double*)q(2), q(6), gt_need - 1); }},
      {"gt_assign/batch_0", A, [&] { return gt(0, 64, 64, 0, 1, 10, q(0), (const double*)q(2), q(6), BIG); }},
      {"gt_assign/M_negative", A, [&] { return gt(0, 64, 64, 2, 1, -1, q(0), (const double*)q(2), q(6), BIG); }},
      {"gt_assign/pad_2", A, [&] { return gt(0, 64, 64, 2, 2, 10, q(0), (const double*)q(2), q(6), BIG); }},
      {"gt_assign/coordinate_type_2", A, [&] { return gt(2, 64, 64, 2, 1, 10, q(0), (const double*)q(2), q(6), BIG); }},
      {"gt_assign/null_lines", A, [&] { return gt(0, 64, 64, 2, 1, 10, nullptr, (const double*)q(2), q(6), BIG); }},
      {"gt_assign/null_homographies", A, [&] { return gt(0, 64, 64, 2, 1, 10, q(0), nullptr, q(6), BIG); }},
      // the backward passes (short workspaces are LINETR_E_ARG there)
      {"linear_backward/short", A, [&] { return linbwd(100, 256, 256, 256, qf(0), qf(4), q(6), linetr_linear_backward_workspace_bytes(100, 256, 256) - 1); }},
      {"linear_backward/rows_0", A, [&] { return linbwd(0, 256, 256, 256, qf(0), qf(4), q(6), BIG); }},
      {"linear_backward/N_not_64k", A, [&] { return linbwd(100, 100, 256, 256, qf(0), qf(4), q(6), BIG); }},
      {"linear_backward/stride_below_width", A, [&] { return linbwd(100, 256, 256, 252, qf(0), qf(4), q(6), BIG); }},
      {"linear_backward/null_input", A, [&] { return linbwd(100, 256, 256, 256, nullptr, qf(4), q(6), BIG); }},
      {"linear_backward/gradient_without_workspace", A, [&] { return linbwd(100, 256, 256, 256, qf(0), qf(4), nullptr, BIG); }},
      {"linear_backward/misaligned_input", A, [&] { return linbwd(100, 256, 256, 256, off(0, 4), qf(4), q(6), BIG); }},
      {"head_backward/short", A, [&] { return headb(100, qf(0), qf(2), q(7), linetr_head_backward_workspace_bytes(100) - 1); }},
      {"head_backward/rows_0", A, [&] { return headb(0, qf(0), qf(2), q(7), BIG); }},
      {"head_backward/null_bias", A, [&] { return headb(100, qf(0), nullptr, q(7), BIG); }},
      {"bn_forward/short", A, [&] { return bnf(100, 256, 0, 1e-5f, qf(0), qf(3), q(6), linetr_bn_forward_workspace_bytes(100, 256) - 1); }},
      {"bn_forward/channels_beyond", A, [&] { return bnf(100, 516, 0, 1e-5f, qf(0), qf(3), q(6), BIG); }},
      {"bn_forward/mode_2", A, [&] { return bnf(100, 256, 2, 1e-5f, qf(0), qf(3), q(6), BIG); }},
      {"bn_forward/eps_0", A, [&] { return bnf(100, 256, 0, 0.f, qf(0), qf(3), q(6), BIG); }},
      {"bn_forward/null_input", A, [&] { return bnf(100, 256, 0, 1e-5f, nullptr, qf(3), q(6), BIG); }},
      {"bn_forward/eval_without_running", A, [&] { return bnf(100, 256, 1, 1e-5f, qf(0), nullptr, q(6), BIG); }},
      {"bn_forward/misaligned_input", A, [&] { return bnf(100, 256, 0, 1e-5f, off(0, 4), qf(3), q(6), BIG); }},
      {"bn_backward/short", A, [&] { return bnb(100, 256, 0, 256, qf(0), q(7), linetr_bn_backward_workspace_bytes(100, 256) - 1); }},
      {"bn_backward/channels_not_4k", A, [&] { return bnb(100, 254, 0, 256, qf(0), q(7), BIG); }},
      {"bn_backward/stride_below_width", A, [&] { return bnb(100, 256, 0, 252, qf(0), q(7), BIG); }},
      {"bn_backward/null_workspace", A, [&] { return bnb(100, 256, 0, 256, qf(0), nullptr, BIG); }},
      {"layer_norm_backward/short", A, [&] { return lnb(100, 256, 256, qf(0), q(7), linetr_layer_norm_backward_workspace_bytes(100, 256) - 1); }},
      {"layer_norm_backward/width_not_256", A, [&] { return lnb(100, 128, 256, qf(0), q(7), BIG); }},
      {"layer_norm_backward/stride_not_4k", A, [&] { return lnb(100, 256, 258, qf(0), q(7), BIG); }},
      {"layer_norm_backward/null_input", A, [&] { return lnb(100, 256, 256, nullptr, q(7), BIG); }},
      {"layer_norm_backward/sums_without_workspace", A, [&] { return lnb(100, 256, 256, qf(0), nullptr, BIG); }},
      {"input_layer_backward/short", A, [&] { return inb(100, 32, 4, qf(0), q(7), linetr_input_layer_backward_workspace_bytes(100, 32, 4) - 1); }},
      {"input_layer_backward/inputs_9", A, [&] { return inb(100, 32, 9, qf(0), q(7), BIG); }},
      {"input_layer_backward/null_input", A, [&] { return inb(100, 32, 4, nullptr, q(7), BIG); }},
      {"token_assemble_backward/short", A, [&] { return tab(100, 21, qf(0), q(7), linetr_token_assemble_backward_workspace_bytes(100) - 1); }},
      {"token_assemble_backward/tokens_0", A, [&] { return tab(100, 0, qf(0), q(7), BIG); }},
      {"token_assemble_backward/null_gradient", A, [&] { return tab(100, 21, nullptr, q(7), BIG); }},
      // the forward halves and the rest of the training pairs: shapes out of range, null and misaligned pointers, the dropout state
      {"linear_forward/K_not_32k", A, [&] { return linetr_linear_forward(nullptr, qf(0), 256, qf(1), qf(2), 100, 256, 100, 0, qf(3), 256, nullptr); }},
      {"linear_forward/act_2", A, [&] { return linetr_linear_forward(nullptr, qf(0), 256, qf(1), qf(2), 100, 256, 256, 2, qf(3), 256, nullptr); }},
      {"linear_forward/null_weight", A, [&] { return linetr_linear_forward(nullptr, qf(0), 256, nullptr, qf(2), 100, 256, 256, 0, qf(3), 256, nullptr); }},
      {"linear_forward/misaligned_output", A, [&] { return linetr_linear_forward(nullptr, qf(0), 256, qf(1), qf(2), 100, 256, 256, 0, off(3, 4), 256, nullptr); }},
      {"head_forward/rows_0", A, [&] { return linetr_head_forward(nullptr, qf(0), qf(1), qf(2), 0, qf(3), nullptr); }},
      {"head_forward/null_output", A, [&] { return linetr_head_forward(nullptr, qf(0), qf(1), qf(2), 100, nullptr, nullptr); }},
      {"head_forward/misaligned_input", A, [&] { return linetr_head_forward(nullptr, off(0, 8), qf(1), qf(2), 100, qf(3), nullptr); }},
      {"sig_attention_forward/no_images", A, [&] { return linetr_sig_attention_forward(nullptr, qf(0), 256, qf(1), 256, qf(2), 256, qi(3), 0, 100, qf(4), 256, qf(5), nullptr); }},
      {"sig_attention_forward/stride_below_256", A, [&] { return linetr_sig_attention_forward(nullptr, qf(0), 252, qf(1), 256, qf(2), 256, qi(3), 2, 100, qf(4), 256, qf(5), nullptr); }},
      {"sig_attention_forward/null_prefix", A, [&] { return linetr_sig_attention_forward(nullptr, qf(0), 256, qf(1), 256, qf(2), 256, nullptr, 2, 100, qf(4), 256, qf(5), nullptr); }},
      {"sig_attention_backward/short", A, [&] { return linetr_sig_attention_backward(nullptr, qf(0), 256, qf(1), 256, qf(2), 256, qf(3), 256, qf(4), qf(5), 256, qi(6), 2, 100, qf(7), 256,
                                                                                     qf(8), 256, qf(9), 256, q(10), linetr_sig_attention_backward_workspace_bytes(100) - 1, nullptr); }},
      {"sig_attention_backward/N_negative", A, [&] { return linetr_sig_attention_backward(nullptr, qf(0), 256, qf(1), 256, qf(2), 256, qf(3), 256, qf(4), qf(5), 256, qi(6), 2, -1, qf(7), 256,
                                                                                          qf(8), 256, qf(9), 256, q(10), BIG, nullptr); }},
      {"sig_attention_backward/null_workspace", A, [&] { return linetr_sig_attention_backward(nullptr, qf(0), 256, qf(1), 256, qf(2), 256, qf(3), 256, qf(4), qf(5), 256, qi(6), 2, 100, qf(7),
                                                                                              256, qf(8), 256, qf(9), 256, nullptr, BIG, nullptr); }},
      {"cls_pool_train_forward/tokens_0", A, [&] { return linetr_cls_pool_train_forward(nullptr, qf(0), 256, qf(1), 1024, 10, 0, qf(2), qf(3), nullptr); }},
      {"cls_pool_train_forward/stride_below_1024", A, [&] { return linetr_cls_pool_train_forward(nullptr, qf(0), 256, qf(1), 1020, 10, 21, qf(2), qf(3), nullptr); }},
      {"cls_pool_train_forward/null_statistics", A, [&] { return linetr_cls_pool_train_forward(nullptr, qf(0), 256, qf(1), 1024, 10, 21, qf(2), nullptr, nullptr); }},
      {"cls_pool_train_backward/segments_negative", A, [&] { return linetr_cls_pool_train_backward(nullptr, qf(0), 256, qf(1), 1024, qf(2), qf(3), qf(4), -1, 21, qf(5), 256, qf(6), 1024, nullptr); }},
      {"cls_pool_train_backward/null_gradient", A, [&] { return linetr_cls_pool_train_backward(nullptr, qf(0), 256, qf(1), 1024, qf(2), qf(3), nullptr, 10, 21, qf(5), 256, qf(6), 1024, nullptr); }},
      {"layer_norm_forward/width_not_256", A, [&] { return linetr_layer_norm_forward(nullptr, qf(0), 256, nullptr, 0, qf(1), qf(2), 1e-6f, 100, 128, qf(3), 256, qf(4), nullptr); }},
      {"layer_norm_forward/eps_0", A, [&] { return linetr_layer_norm_forward(nullptr, qf(0), 256, nullptr, 0, qf(1), qf(2), 0.f, 100, 256, qf(3), 256, qf(4), nullptr); }},
      {"layer_norm_forward/null_beta", A, [&] { return linetr_layer_norm_forward(nullptr, qf(0), 256, nullptr, 0, qf(1), nullptr, 1e-6f, 100, 256, qf(3), 256, qf(4), nullptr); }},
      {"gelu_forward/channels_not_4k", A, [&] { return linetr_gelu_forward(nullptr, qf(0), 1024, 100, 1022, qf(1), 1024, nullptr); }},
      {"gelu_forward/null_output", A, [&] { return linetr_gelu_forward(nullptr, qf(0), 1024, 100, 1024, nullptr, 1024, nullptr); }},
      {"gelu_backward/null_gradient", A, [&] { return linetr_gelu_backward(nullptr, qf(0), 1024, nullptr, 1024, 100, 1024, qf(2), 1024, nullptr); }},
      {"gelu_backward/stride_below_width", A, [&] { return linetr_gelu_backward(nullptr, qf(0), 1024, qf(1), 1020, 100, 1024, qf(2), 1024, nullptr); }},
      {"input_layer_forward/outputs_68", A, [&] { return linetr_input_layer_forward(nullptr, qf(0), 4, qf(1), qf(2), 100, 68, 4, qf(3), 68, nullptr); }},
      {"input_layer_forward/null_weight", A, [&] { return linetr_input_layer_forward(nullptr, qf(0), 4, nullptr, qf(2), 100, 32, 4, qf(3), 32, nullptr); }},
      {"input_layer_forward/misaligned_output", A, [&] { return linetr_input_layer_forward(nullptr, qf(0), 4, qf(1), qf(2), 100, 32, 4, off(3, 4), 32, nullptr); }},
      {"token_assemble_forward/segments_negative", A, [&] { return linetr_token_assemble_forward(nullptr, qf(0), qf(1), qf(2), -1, 21, qf(3), nullptr); }},
      {"token_assemble_forward/null_class_token", A, [&] { return linetr_token_assemble_forward(nullptr, qf(0), qf(1), nullptr, 10, 21, qf(3), nullptr); }},
      {"dropout_factors/null_state", A, [&] { return linetr_dropout_factors(nullptr, nullptr, 1, 10, 64, qf(0), nullptr); }},
      {"dropout_factors/site_3", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) { return linetr_dropout_factors(nullptr, d, 3, 10, 64, qf(0), nullptr); }); }},
      {"dropout_factors/scale_below_1", A, [&] { return dropout([](LinetrDropout& d) { d.scale = 0.5f; }, [&](const LinetrDropout* d) { return linetr_dropout_factors(nullptr, d, 1, 10, 64, qf(0), nullptr); }); }},
      {"dropout_factors/scale_nan", A, [&] { return dropout([&](LinetrDropout& d) { d.scale = (float)NaN; }, [&](const LinetrDropout* d) { return linetr_dropout_factors(nullptr, d, 1, 10, 64, qf(0), nullptr); }); }},
      {"dropout_factors/inner_0", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) { return linetr_dropout_factors(nullptr, d, 1, 10, 0, qf(0), nullptr); }); }},
      {"dropout_factors/misaligned_output", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) { return linetr_dropout_factors(nullptr, d, 1, 10, 64, off(0, 4), nullptr); }); }},
      {"cls_pool_dropout_forward/null_state", A, [&] { return linetr_cls_pool_dropout_forward(nullptr, qf(0), 256, qf(1), 1024, 10, 21, nullptr, qf(2), qf(3), qf(4), nullptr); }},
      {"cls_pool_dropout_forward/scale_below_1", A, [&] { return dropout([](LinetrDropout& d) { d.scale = 0.25f; }, [&](const LinetrDropout* d) {
         return linetr_cls_pool_dropout_forward(nullptr, qf(0), 256, qf(1), 1024, 10, 21, d, qf(2), qf(3), qf(4), nullptr); }); }},
      {"cls_pool_dropout_forward/null_kept", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) {
         return linetr_cls_pool_dropout_forward(nullptr, qf(0), 256, qf(1), 1024, 10, 21, d, qf(2), nullptr, qf(4), nullptr); }); }},
      {"cls_pool_dropout_backward/null_state", A, [&] { return linetr_cls_pool_dropout_backward(nullptr, qf(0), 256, qf(1), 1024, qf(2), qf(3), qf(4), qf(5), nullptr, 10, 21, nullptr, qf(6), 256,
                                                                                                qf(7), 1024, nullptr); }},
      {"cls_pool_dropout_backward/misaligned_kept", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) {
         return linetr_cls_pool_dropout_backward(nullptr, qf(0), 256, qf(1), 1024, qf(2), qf(3), off(4, 4), qf(5), nullptr, 10, 21, d, qf(6), 256, qf(7), 1024, nullptr); }); }},
      {"layer_norm_dropout_forward/null_state", A, [&] { return linetr_layer_norm_dropout_forward(nullptr, qf(0), 256, nullptr, 0, qf(1), qf(2), 1e-6f, 100, 256, nullptr, 1, qf(3), 256, qf(4), nullptr); }},
      {"layer_norm_dropout_forward/site_negative", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) {
         return linetr_layer_norm_dropout_forward(nullptr, qf(0), 256, nullptr, 0, qf(1), qf(2), 1e-6f, 100, 256, d, -1, qf(3), 256, qf(4), nullptr); }); }},
      {"layer_norm_dropout_backward/scale_inf", A, [&] { return dropout([](LinetrDropout& d) { d.scale = std::numeric_limits<float>::infinity(); }, [&](const LinetrDropout* d) {
         return linetr_layer_norm_dropout_backward(nullptr, qf(0), 256, nullptr, 0, qf(1), qf(2), qf(3), 256, 100, 256, d, 1, qf(4), 256, nullptr, 0, qf(5), qf(6), q(7), BIG, nullptr); }); }},
      {"layer_norm_dropout_backward/short", A, [&] { return dropout([](LinetrDropout&) {}, [&](const LinetrDropout* d) {
         return linetr_layer_norm_dropout_backward(nullptr, qf(0), 256, nullptr, 0, qf(1), qf(2), qf(3), 256, 100, 256, d, 1, qf(4), 256, nullptr, 0, qf(5), qf(6), q(7),
                                                   linetr_layer_norm_backward_workspace_bytes(100, 256) - 1, nullptr); }); }},
  };
  run_refusals(t, "refusals_tables_out.txt");
  CHECK(block.all_bytes(0), "a refused call wrote into the block its pointers came from");
  return 0;
}

int cmd_malformed() {
  const double NaN = std::numeric_limits<double>::quiet_NaN(), Inf = std::numeric_limits<double>::infinity();
  const int H = 480, Wd = 640, A = LINETR_E_ARG, OK = LINETR_OK;
  // 200 well-formed lines: 40 px long horizontal segments on a grid, all inside an H x Wd image
  const int K = 200;
  Heap<double> lines((size_t)K * 6);
  for (int k = 0; k < K; ++k) {
    double* l = lines.p + 6 * k;
    l[0] = 20.0 + 50.0 * (k % 10); l[1] = 20.0 + 20.0 * (k / 10); l[2] = l[0] + 40.0; l[3] = l[1]; l[4] = 30.0 + 0.01 * k; l[5] = 0.0;
  }
  Heap<LinetrLineRec> recs((size_t)K, 0xAB);
  Heap<int32_t> cu_k(4, 0xCD), cu_n(4, 0xCD), ko(1), no(1);
  Heap<double> vm((size_t)H * Wd);
  for (size_t i = 0; i < vm.n; ++i) vm.p[i] = 1.0;
  Heap<const double*> vms(2);
  vms.p[0] = vm.p; vms.p[1] = vm.p;
  auto table3 = [](int a, int b, int c) { Heap<int32_t> o(3); o.p[0] = a; o.p[1] = b; o.p[2] = c; return o; };
  auto table4 = [](int a, int b, int c, int d) { Heap<int32_t> o(4); o.p[0] = a; o.p[1] = b; o.p[2] = c; o.p[3] = d; return o; };
  const Heap<int32_t> good = table3(0, 100, 200), decreasing = table3(0, 200, 100), negative = table3(0, -5, 200), negative_first = table3(-1, 100, 200),
                      overlapping = table4(0, 120, 80, 200);
  auto batch = [&](const int32_t* off, int B, int height, int width, int border, int max_k, const double* const* masks, double td, int T, int nt,
                   LinetrLineRec* out, int cap) {
    return linetr_prefilter_batch(lines.p, off, B, height, width, border, 16.0, max_k, masks, td, T, nt, out, cap, cu_k.p, cu_n.p);
  };
  auto single = [&](const double* L, int k, int height, int width, int border, int max_k, const double* mask, double td, int T, LinetrLineRec* out, int cap) {
    return linetr_prefilter(L, k, height, width, border, 16.0, max_k, mask, td, T, 0, 0, 0, out, cap, ko.p, no.p);
  };
  // one line with a poisoned field, for the NaN / infinity rows: the reference's comparisons drop it (LINETR_OK, no survivor)
  auto poisoned = [&](int field, double v) { Heap<double> l(6); memcpy(l.p, lines.p, 48); l.p[field] = v; return l; };
  auto dropped = [&](int field, double v) {
    Heap<double> l = poisoned(field, v);
    const int code = single(l.p, 1, H, Wd, 8, 512, nullptr, 8.0, 21, recs.p, 1);
    return code != OK ? code : ko.p[0] == 0 ? OK : -100;
  };
  // caller-packed lines (linetr_pack_lines takes them as they are)
  auto pack = [&](double x1, double len, double td, int T, int n) {
    Heap<double> kl((size_t)n * 4), ln((size_t)n), an((size_t)n * 2);
    for (int i = 0; i < n; ++i) { kl.p[4 * i + 2] = x1; ln.p[i] = len; an.p[2 * i] = 1.0; }
    Heap<LinetrLineRec> out((size_t)n, 0xAB);
    return linetr_pack_lines(kl.p, ln.p, an.p, n, td, T, 0, 0, 0, out.p, no.p);
  };
  Heap<double> attr_lines(8);
  for (int i = 0; i < 8; ++i) attr_lines.p[i] = 20.0 + 30.0 * i;
  auto attributes = [&](int n, int poisoned_at, double v, int max_sublines = 10) {
    Heap<double> l(8), kl(8), ln(2), an(4);
    memcpy(l.p, attr_lines.p, 64);
    if (poisoned_at >= 0) l.p[poisoned_at] = v;
    const int code = linetr_find_line_attributes(l.p, n, 16.0, max_sublines, kl.p, ln.p, an.p, no.p);
    return code != OK || max_sublines >= 0 ? code : no.p[0] == 0 ? OK : -100;
  };
  std::vector<Refusal> t = {
      {"batch/well_formed", OK, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/offsets_decreasing", A, [&] { return batch(decreasing.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/offsets_negative", A, [&] { return batch(negative.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/offsets_negative_first", A, [&] { return batch(negative_first.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/offsets_overlapping", A, [&] { return batch(overlapping.p, 3, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/offsets_null", A, [&] { return batch(nullptr, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/negative_images", A, [&] { return batch(good.p, -1, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/records_null", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, nullptr, K); }},
      {"batch/capacity_negative", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, -1); }},
      {"batch/threads_negative", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, 8.0, 21, -1, recs.p, K); }},
      {"batch/border_negative", A, [&] { return batch(good.p, 2, H, Wd, -8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/border_negative_with_mask", A, [&] { return batch(good.p, 2, H, Wd, -8, 512, vms.p, 8.0, 21, 1, recs.p, K); }},
      {"batch/height_negative", A, [&] { return batch(good.p, 2, -H, Wd, 8, 512, nullptr, 8.0, 21, 1, recs.p, K); }},
      {"batch/width_negative", A, [&] { return batch(good.p, 2, H, -Wd, 8, 512, vms.p, 8.0, 21, 1, recs.p, K); }},
      {"batch/token_distance_0", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, 0.0, 21, 1, recs.p, K); }},
      {"batch/token_distance_negative", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, -8.0, 21, 1, recs.p, K); }},
      {"batch/token_distance_nan", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, NaN, 21, 1, recs.p, K); }},
      {"batch/max_tokens_0", A, [&] { return batch(good.p, 2, H, Wd, 8, 512, nullptr, 8.0, 0, 1, recs.p, K); }},
      {"batch/token_distance_0_without_lines", A, [&] { return batch(table3(0, 0, 0).p, 2, H, Wd, 8, 512, nullptr, 0.0, 21, 1, recs.p, K); }},
      {"batch/max_keylines_int_min", OK, [&] { const int c = batch(good.p, 2, H, Wd, 8, INT32_MIN, nullptr, 8.0, 21, 1, recs.p, K); return c != OK ? c : cu_k.p[2] == 0 ? OK : -100; }},
      {"single/negative_lines", A, [&] { return single(lines.p, -1, H, Wd, 8, 512, nullptr, 8.0, 21, recs.p, K); }},
      {"single/lines_null", A, [&] { return single(nullptr, 5, H, Wd, 8, 512, nullptr, 8.0, 21, recs.p, K); }},
      {"single/records_null", A, [&] { return single(lines.p, K, H, Wd, 8, 512, nullptr, 8.0, 21, nullptr, K); }},
      {"single/capacity_negative", A, [&] { return single(lines.p, K, H, Wd, 8, 512, nullptr, 8.0, 21, recs.p, -K); }},
      {"single/border_negative_with_mask", A, [&] { return single(lines.p, K, H, Wd, -1, 512, vm.p, 8.0, 21, recs.p, K); }},
      {"single/height_negative", A, [&] { return single(lines.p, K, -1, Wd, 8, 512, nullptr, 8.0, 21, recs.p, K); }},
      {"single/token_distance_nan", A, [&] { return single(lines.p, K, H, Wd, 8, 512, nullptr, NaN, 21, recs.p, K); }},
      {"single/max_tokens_0", A, [&] { return single(lines.p, K, H, Wd, 8, 512, nullptr, 8.0, 0, recs.p, K); }},
      {"single/max_keylines_int_min", OK, [&] { const int c = single(lines.p, K, H, Wd, 8, INT32_MIN, nullptr, 8.0, 21, recs.p, K); return c != OK ? c : ko.p[0] == 0 ? OK : -100; }},
      {"single/counts_null", A, [&] { return linetr_prefilter(lines.p, K, H, Wd, 8, 16.0, 512, nullptr, 8.0, 21, 0, 0, 0, recs.p, K, nullptr, no.p); }},
      // NaN and infinity in a line: the reference's comparisons drop the line; an infinite length that survives them is refused
      {"line/x_nan", OK, [&] { return dropped(0, NaN); }},
      {"line/y_nan", OK, [&] { return dropped(3, NaN); }},
      {"line/x_inf", OK, [&] { return dropped(2, Inf); }},
      {"line/y_minus_inf", OK, [&] { return dropped(1, -Inf); }},
      {"line/length_nan", OK, [&] { return dropped(4, NaN); }},
      {"line/octave_nan", OK, [&] { return dropped(5, NaN); }},
      {"line/octave_minus_inf", OK, [&] { return dropped(5, -Inf); }},
      {"line/length_inf", A, [&] { return dropped(4, Inf); }},
      {"line/octave_inf", A, [&] { return dropped(5, Inf); }},
      {"line/octave_huge", A, [&] { return dropped(5, 1e300); }},
      {"line/x_nan_with_mask", OK, [&] { Heap<double> l = poisoned(0, NaN); const int c = single(l.p, 1, H, Wd, 8, 512, vm.p, 8.0, 21, recs.p, 1); return c != OK ? c : ko.p[0] == 0 ? OK : -100; }},
      // linetr_pack_lines takes the caller's lines as they are
      {"pack/negative_lines", A, [&] { return linetr_pack_lines(lines.p, lines.p, lines.p, -1, 8.0, 21, 0, 0, 0, recs.p, no.p); }},
      {"pack/records_null", A, [&] { return linetr_pack_lines(lines.p, lines.p, lines.p, 1, 8.0, 21, 0, 0, 0, nullptr, no.p); }},
      {"pack/length_nan", A, [&] { return pack(40.0, NaN, 8.0, 21, 1); }},
      {"pack/length_inf", A, [&] { return pack(40.0, Inf, 8.0, 21, 1); }},
      {"pack/length_negative", A, [&] { return pack(40.0, -30.0, 8.0, 21, 1); }},
      {"pack/end_point_nan", LINETR_E_ASSERT, [&] { return pack(NaN, 30.0, 8.0, 21, 1); }},
      {"pack/longer_than_the_segment", LINETR_E_ASSERT, [&] { return pack(40.0, 200.0, 8.0, 21, 1); }},
      {"pack/token_distance_0", A, [&] { return pack(40.0, 30.0, 0.0, 21, 1); }},
      {"pack/token_distance_nan", A, [&] { return pack(40.0, 30.0, NaN, 21, 1); }},
      {"pack/max_tokens_negative", A, [&] { return pack(40.0, 30.0, 8.0, -1, 1); }},
      {"pack/token_distance_0_without_lines", A, [&] { return pack(40.0, 30.0, 0.0, 21, 0); }},
      {"pack/counts_beyond_int32", A, [&] { return pack(1e8, 7.9e7, 8.0, 1, 300); }},
      // pseudo lines and their attributes
      {"pseudo/negative_lines", A, [&] { return linetr_make_pseudo_lines(1, 0, -1, 480.0, 640.0, 16.0, attr_lines.p); }},
      {"pseudo/lines_null", A, [&] { return linetr_make_pseudo_lines(1, 0, 2, 480.0, 640.0, 16.0, nullptr); }},
      {"pseudo/seed_beyond_32_bits", A, [&] { return linetr_make_pseudo_lines(uint64_t(1) << 32, 0, 2, 480.0, 640.0, 16.0, attr_lines.p); }},
      {"pseudo/image_negative", A, [&] { return linetr_make_pseudo_lines(1, -1, 2, 480.0, 640.0, 16.0, attr_lines.p); }},
      {"pseudo/shape_nan", A, [&] { return linetr_make_pseudo_lines(1, 0, 2, NaN, 640.0, 16.0, attr_lines.p); }},
      {"pseudo/shape_without_room", A, [&] { return linetr_make_pseudo_lines(1, 0, 2, 61.0, 640.0, 16.0, attr_lines.p); }},
      {"pseudo/min_length_nan", A, [&] { return linetr_make_pseudo_lines(1, 0, 2, 480.0, 640.0, NaN, attr_lines.p); }},
      {"pseudo/min_length_160", A, [&] { return linetr_make_pseudo_lines(1, 0, 2, 480.0, 640.0, 160.0, attr_lines.p); }},
      {"pseudo/shape_inf", OK, [&] { Heap<double> l(8, 0xAB); return linetr_make_pseudo_lines(1, 0, 2, Inf, 640.0, 16.0, l.p); }},
      {"attributes/well_formed", OK, [&] { return attributes(2, -1, 0.0); }},
      {"attributes/negative_lines", A, [&] { return attributes(-2, -1, 0.0); }},
      {"attributes/coordinate_nan", A, [&] { return attributes(2, 5, NaN); }},
      {"attributes/coordinate_inf", A, [&] { return attributes(2, 0, Inf); }},
      {"attributes/count_null", A, [&] { Heap<double> kl(8), ln(2), an(4); return linetr_find_line_attributes(attr_lines.p, 2, 16.0, 10, kl.p, ln.p, an.p, nullptr); }},
      {"attributes/max_sublines_int_min", OK, [&] { return attributes(2, -1, 0.0, INT32_MIN); }},
      // the weight preparation's table of tensors
      {"prepare/config_null", A, [&] { int64_t nf; int32_t ne; return linetr_debug_prepare(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, &nf, &ne); }},
      {"prepare/negative_tensors", A, [&] {
         LinetrModelConfig c{256, 4, 1024, 1, 1, {32, 64, 128, 256}, 480, 640, 0};
         Heap<const char*> names(1); Heap<const float*> data(1); Heap<int64_t> numel(1);
         int64_t nf; int32_t ne;
         return linetr_debug_prepare(&c, -1, names.p, data.p, numel.p, nullptr, 0, nullptr, 0, &nf, &ne); }},
      {"prepare/name_null", A, [&] {
         LinetrModelConfig c{256, 4, 1024, 1, 1, {32, 64, 128, 256}, 480, 640, 0};
         Heap<const char*> names(1); Heap<const float*> data(1); Heap<int64_t> numel(1);
         int64_t nf; int32_t ne;
         return linetr_debug_prepare(&c, 1, names.p, data.p, numel.p, nullptr, 0, nullptr, 0, &nf, &ne); }},
      {"prepare/capacity_negative", A, [&] {
         LinetrModelConfig c{256, 4, 1024, 1, 1, {32, 64, 128, 256}, 480, 640, 0};
         Heap<const char*> names(1); Heap<const float*> data(1); Heap<int64_t> numel(1); Heap<float> image(1);
         int64_t nf; int32_t ne;
         return linetr_debug_prepare(&c, 0, names.p, data.p, numel.p, image.p, -1, nullptr, 0, &nf, &ne); }},
  };
  run_refusals(t, "malformed_out.txt");
  return 0;
}

// ============================================================================================================================
// threads
// ============================================================================================================================

struct ThreadJob {
  int id = 0;
  int failures = 0;
  std::string note;
};

pthread_barrier_t g_start;

// 32 images of 40 lines each; thread `id` plants equal lengths into its own set of images
void thread_main(ThreadJob* job) {
  const int id = job->id, B = 32, per = 40, H = 480, Wd = 640, ROUNDS = 50;
  Heap<double> lines((size_t)B * per * 6);
  Heap<int32_t> off((size_t)B + 1);
  uint64_t s = 0x9E3779B97F4A7C15ull * (uint64_t)(id + 1);
  auto rnd = [&] { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; };
  for (int i = 0; i <= B; ++i) off.p[i] = i * per;
  for (int k = 0; k < B * per; ++k) {
    double* l = lines.p + 6 * k;
    const double len = 20.0 + 180.0 * rnd(), ang = 6.283185307179586 * rnd();
    // every value a float32, the detector's type (the oracle's key-line objects hold float32)
    l[0] = (float)(10.0 + (Wd - 20.0) * rnd()); l[1] = (float)(10.0 + (H - 20.0) * rnd());
    l[2] = (float)(l[0] + len * std::cos(ang)); l[3] = (float)(l[1] + len * std::sin(ang));
    l[4] = (float)(std::hypot(l[2] - l[0], l[3] - l[1]) * (0.5 + 0.45 * rnd())); l[5] = 0.0;   // a detector length below the geometric one
  }
  std::vector<int32_t> want_tied;
  for (int i = 0; i < B; ++i)
    if ((i + id) % 4 == 0 || i == 3 * id + 1) {                       // this thread's own set of tied images
      double* a = lines.p + 6 * ((size_t)i * per + 2);
      double* b = lines.p + 6 * ((size_t)i * per + 17);
      a[0] = 100.0; a[1] = 100.0 + id; a[2] = 300.0; a[3] = 100.0 + id; a[4] = 150.0;
      b[0] = 120.0; b[1] = 200.0 + id; b[2] = 320.0; b[3] = 200.0 + id; b[4] = 150.0;
      want_tied.push_back(i);
    }
  const int K = B * per;
  Heap<LinetrLineRec> ref((size_t)K, 0xAB), got((size_t)K, 0xAB);
  Heap<int32_t> ck((size_t)B + 1), cn((size_t)B + 1), ck2((size_t)B + 1), cn2((size_t)B + 1), tied((size_t)B);
  const Heap<int32_t> bad_off = [&] { Heap<int32_t> o(3); o.p[0] = 0; o.p[1] = 200; o.p[2] = 100; return o; }();
  auto fail_here = [&](const std::string& what) { ++job->failures; if (job->note.empty()) job->note = what; };
  pthread_barrier_wait(&g_start);                                     // the pool's first use is contended too
  for (int round = 0; round < ROUNDS; ++round) {
    int code = linetr_prefilter_batch(lines.p, off.p, B, H, Wd, 8, 16.0, 512, nullptr, 8.0, 21, 8, got.p, K, ck2.p, cn2.p);
    if (code != LINETR_OK) { fail_here("pooled call failed: " + std::string(last_error())); continue; }
    const int32_t n_tied = linetr_prefilter_tied_images(tied.p, B);
    if (n_tied != (int32_t)want_tied.size() || memcmp(tied.p, want_tied.data(), want_tied.size() * 4)) fail_here("another thread's tied images were read back");
    if (round == 0 || id % 2) {                                        // the n_threads = 1 result: once, or (odd threads) every round
      code = linetr_prefilter_batch(lines.p, off.p, B, H, Wd, 8, 16.0, 512, nullptr, 8.0, 21, 1, ref.p, K, ck.p, cn.p);
      if (code != LINETR_OK) { fail_here("single-thread call failed"); continue; }
    }
    const size_t k = (size_t)ck.p[B];
    if (memcmp(ck.p, ck2.p, ck.bytes()) || memcmp(cn.p, cn2.p, cn.bytes()) || memcmp(ref.p, got.p, k * sizeof(LinetrLineRec)))
      fail_here("the pooled result differs from n_threads = 1 in round " + std::to_string(round));
    if (id < 2) {                                                      // two threads also fail, each in its own way, and read their own message
      if (id == 0) {
        code = linetr_prefilter_batch(lines.p, bad_off.p, 2, H, Wd, 8, 16.0, 512, nullptr, 8.0, 21, 8, got.p, K, ck2.p, cn2.p);
        if (code != LINETR_E_ARG || !strstr(last_error(), "offset")) fail_here("thread 0: status " + std::to_string(code) + ", message '" + last_error() + "'");
      } else {
        code = linetr_prefilter_batch(lines.p, off.p, B, H, Wd, 8, 16.0, 512, nullptr, 8.0, 21, 8, got.p, 5, ck2.p, cn2.p);
        if (code != LINETR_E_CAPACITY || !strstr(last_error(), "surviving")) fail_here("thread 1: status " + std::to_string(code) + ", message '" + last_error() + "'");
      }
    }
  }
  if (id == 0) {
    write_bin("thread0_recs.bin", ref.p, (size_t)ck.p[B] * sizeof(LinetrLineRec));
    write_bin("thread0_lines.bin", lines.p, lines.bytes());
    write_bin("thread0_cu_k.bin", ck.p, ck.bytes());
  }
}

int cmd_threads() {
  const int N = 4;
  pthread_barrier_init(&g_start, nullptr, N);
  ThreadJob jobs[N];
  std::vector<std::thread> th;
  for (int i = 0; i < N; ++i) { jobs[i].id = i; th.emplace_back(thread_main, &jobs[i]); }
  for (auto& t : th) t.join();
  pthread_barrier_destroy(&g_start);
  for (int i = 0; i < N; ++i) CHECK(jobs[i].failures == 0, "thread %d: %d failures, the first: %s", i, jobs[i].failures, jobs[i].note.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) die("usage: host_driver <prefilter|pseudo|prepare|photo|queries|refusals|malformed|threads> <directory>");
  const std::string cmd = argv[1];
  g_dir = argv[2];
  if (cmd == "prefilter") cmd_prefilter();
  else if (cmd == "pseudo") cmd_pseudo();
  else if (cmd == "prepare") cmd_prepare();
  else if (cmd == "photo") cmd_photo();
  else if (cmd == "queries") cmd_queries();
  else if (cmd == "refusals") { cmd_refusals(); cmd_refusals_tables(); }
  else if (cmd == "malformed") cmd_malformed();
  else if (cmd == "threads") cmd_threads();
  else die("unknown command %s", cmd.c_str());
  if (g_failures) { fprintf(stderr, "host_driver: %d mismatches\n", g_failures); return 1; }
  printf("host_driver %s: ok\n", cmd.c_str());
  return 0;
}
