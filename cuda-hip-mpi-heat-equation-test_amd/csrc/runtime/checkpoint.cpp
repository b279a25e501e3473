// Checkpoint / restart for the native CLI, in the SAME on-disk format as the
// Python driver (utils/checkpoint.py, "heat2d-checkpoint-v2", ckpt.hpp):
//   DIR/step-NNNNNNNNNNNN/rankNNNNN.npy  each rank's owned rows (NumPy v1 header, C order)
//   DIR/step-NNNNNNNNNNNN/meta.json      problem + solver parameters + completed step count
//   DIR/latest                           the newest complete step (atomic commit point)
// so a run can checkpoint from `heat2d --gpus 8` and resume under torchrun
// (or the other way round), on any rank count: restart reads each writer
// file's row range that overlaps this rank's slab. The reference has no
// restart at all (its int.dat / soln*.dat dumps are never read back;
// SURVEY.md §5).
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>

#include "heat2d/capi.h"
#include "heat2d/ckpt.hpp"
#include "heat2d/runtime.hpp"

namespace heat2d {
namespace ckpt {

namespace {

constexpr const char* kFormat = "heat2d-checkpoint-v2";
constexpr const char* kFormatV1 = "heat2d-checkpoint-v1";  // flat layout, still readable

std::string join(const std::string& dir, const std::string& name) { return dir + "/" + name; }

std::string step_name(int64_t step) {
  char b[32];
  std::snprintf(b, sizeof(b), "step-%012lld", (long long)step);
  return b;
}

bool exists(const std::string& p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0;
}

// data of `path` (a file or a directory: its entries) on stable storage
void fsync_path(const std::string& path) {
  const int fd = ::open(path.c_str(), O_RDONLY);
  HEAT2D_REQUIRE(fd >= 0, "cannot open " + path + " to fsync");
  const int rc = ::fsync(fd);
  const int err = errno;  // (close may overwrite it)
  ::close(fd);
  HEAT2D_REQUIRE(rc == 0 || err == EINVAL, "fsync failed on " + path);
}

std::string parent_dir(const std::string& path) {
  const size_t p = path.find_last_of('/');
  return p == std::string::npos ? "." : (p == 0 ? "/" : path.substr(0, p));
}

void write_atomic(const std::string& path, const std::string& text) {
  const std::string tmp = path + ".tmp";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  HEAT2D_REQUIRE(f != nullptr, "cannot write " + tmp);
  const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size() && std::fflush(f) == 0 &&
                  ::fsync(fileno(f)) == 0;
  HEAT2D_REQUIRE(std::fclose(f) == 0 && ok, "error writing " + tmp);
  HEAT2D_REQUIRE(std::rename(tmp.c_str(), path.c_str()) == 0, "cannot publish " + path);
  fsync_path(parent_dir(path));  // the rename itself
}

std::string rank_file(const std::string& dir, int rank) {
  char b[32];
  std::snprintf(b, sizeof(b), "rank%05d.npy", rank);
  return join(dir, b);
}

// closes on every exit path (the REQUIREs below throw)
struct File {
  FILE* f;
  File(const std::string& path, const char* mode) : f(std::fopen(path.c_str(), mode)) {
    HEAT2D_REQUIRE(f != nullptr, "cannot open " + path);
  }
  ~File() {
    if (f) std::fclose(f);
  }
  File(const File&) = delete;
  File& operator=(const File&) = delete;
};

std::string read_text(const std::string& path) {
  File f(path, "rb");
  std::string s;
  char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof(buf), f.f)) > 0) s.append(buf, n);
  return s;
}

// Value of "key" in a flat JSON object (numbers or strings; enough for the
// meta.json both writers produce).
std::string json_value(const std::string& js, const std::string& key) {
  const std::string pat = "\"" + key + "\"";
  size_t p = js.find(pat);
  HEAT2D_REQUIRE(p != std::string::npos, "checkpoint meta.json lacks \"" + key + "\"");
  p = js.find(':', p + pat.size());
  HEAT2D_REQUIRE(p != std::string::npos, "malformed meta.json");
  ++p;
  while (p < js.size() && (js[p] == ' ' || js[p] == '\n' || js[p] == '\t' || js[p] == '\r')) ++p;
  HEAT2D_REQUIRE(p < js.size(), "malformed meta.json");
  if (js[p] == '"') {
    const size_t q = js.find('"', p + 1);
    HEAT2D_REQUIRE(q != std::string::npos, "malformed meta.json string");
    return js.substr(p + 1, q - p - 1);
  }
  size_t q = p;
  while (q < js.size() && js[q] != ',' && js[q] != '}' && js[q] != '\n') ++q;
  return js.substr(p, q - p);
}

struct NpyInfo {
  int64_t rows = 0, cols = 0;
  int64_t planes = 0;  // 3-D arrays: the first extent (rows / cols the other two); 0: 2-D
  int dtype = 1;       // 0 fp32, 1 fp64
  long data_off = 0;   // byte offset of the array data
};

NpyInfo npy_header(FILE* f, const std::string& path) {
  unsigned char head[10];
  HEAT2D_REQUIRE(std::fread(head, 1, 10, f) == 10 && std::memcmp(head, "\x93NUMPY", 6) == 0,
                 path + ": not a .npy file");
  const int major = head[6];
  size_t hlen = 0;
  long off = 0;
  if (major == 1) {
    hlen = (size_t)head[8] | ((size_t)head[9] << 8);
    off = 10;
  } else {
    unsigned char ext[2];
    HEAT2D_REQUIRE(std::fread(ext, 1, 2, f) == 2, path + ": truncated header");
    hlen = (size_t)head[8] | ((size_t)head[9] << 8) | ((size_t)ext[0] << 16) | ((size_t)ext[1] << 24);
    off = 12;
  }
  HEAT2D_REQUIRE(hlen > 0 && hlen < (1u << 20), path + ": bad header length");
  std::string h(hlen, '\0');
  HEAT2D_REQUIRE(std::fread(&h[0], 1, hlen, f) == hlen, path + ": truncated header");
  NpyInfo info;
  info.data_off = off + (long)hlen;
  if (h.find("'<f8'") != std::string::npos) info.dtype = 1;
  else if (h.find("'<f4'") != std::string::npos) info.dtype = 0;
  else fail(__FILE__, __LINE__, path + ": dtype is not little-endian f4/f8");
  HEAT2D_REQUIRE(h.find("'fortran_order': False") != std::string::npos, path + ": Fortran-ordered array");
  const size_t sp = h.find("'shape':");
  HEAT2D_REQUIRE(sp != std::string::npos, path + ": no shape");
  long long r = 0, c = 0;
  HEAT2D_REQUIRE(std::sscanf(h.c_str() + sp, "'shape': (%lld, %lld)", &r, &c) == 2 && r >= 0 && c > 0,
                 path + ": expected a 2-D shape");
  info.rows = r;
  info.cols = c;
  long long a3 = 0, b3 = 0, c3 = 0;
  if (std::sscanf(h.c_str() + sp, "'shape': (%lld, %lld, %lld)", &a3, &b3, &c3) == 3) {
    info.planes = a3;
    info.rows = b3;
    info.cols = c3;
  }
  return info;
}

}  // namespace

// (step, generation) of a step directory name "step-<12 digits>[-<digits>]"
// (generation 0: the bare name; any all-digit suffix counts, the legacy -N
// too); false for anything else. Pruning orders saves by this key, not by
// name: a legacy step-X-7 and a new step-X-000008 compare by their numbers.
static bool step_key(const std::string& n, long long* step, long long* gen) {
  if (n.compare(0, 5, "step-") != 0 || n.size() < 5 + 12) return false;
  for (size_t i = 5; i < 17; ++i)
    if (!std::isdigit((unsigned char)n[i])) return false;
  *step = std::atoll(n.c_str() + 5);
  *gen = 0;
  if (n.size() == 17) return true;
  if (n[17] != '-' || n.size() == 18) return false;
  for (size_t i = 18; i < n.size(); ++i)
    if (!std::isdigit((unsigned char)n[i])) return false;
  *gen = std::atoll(n.c_str() + 18);
  return true;
}

// A name no earlier save of this step used, ordered after all of them (and
// before the next step) by step_key: `base` for the first save, then
// base-000001, base-000002, ... one past the highest generation present
// (legacy -N suffixes included) — never a gap a pruned generation left.
std::string step_dir_name(const std::string& dir, int64_t step) {
  const std::string base = step_name(step);
  bool any = false;
  long long gmax = 0;
  if (DIR* d = ::opendir(dir.c_str())) {
    while (dirent* e = ::readdir(d)) {
      long long st = 0, g = 0;
      if (!step_key(e->d_name, &st, &g) || st != (long long)step) continue;
      any = true;
      gmax = std::max(gmax, g);
    }
    ::closedir(d);
  }
  if (!any) return base;
  char b[16];
  std::snprintf(b, sizeof(b), "-%06lld", gmax + 1);
  return base + b;
}

void write_rank(const std::string& dir, const std::string& name, int rank, Solver& s) {
  ::mkdir(dir.c_str(), 0755);  // all ranks may race on it: EEXIST is fine
  const std::string sd = join(dir, name);
  ::mkdir(sd.c_str(), 0755);
  const SlabLayout& L = s.layout();
  std::vector<char> host((size_t)(L.nrows * L.ncols) * dtype_size(s.dtype()));
  s.download(host.data(), L.ncols);
  const std::string path = rank_file(sd, rank);
  if (heat2d_write_npy(path.c_str(), (int)s.dtype(), host.data(), L.nrows, L.ncols, L.ncols))
    fail(__FILE__, __LINE__, heat2d_last_error());
  fsync_path(path);
}

namespace {
const char* const kRobinKeys[4] = {"x_lo", "x_hi", "y_lo", "y_hi"};
// " \"robin\": {\"x_lo\": [\"0x1.ap-1\", \"0x1.7ae148p-2\"], ...},\n" ("" without a recorded side)
std::string robin_json(const Meta& m) {
  if (!m.robin_sides) return "";
  std::string o = " \"robin\": {";
  bool first = true;
  for (int k = 0; k < 4; ++k) {
    if (!(m.robin_sides >> k & 1)) continue;
    char b[128];
    std::snprintf(b, sizeof(b), "%s\"%s\": [\"%a\", \"%a\"]", first ? "" : ", ", kRobinKeys[k], m.robin[2 * k], m.robin[2 * k + 1]);
    o += b;
    first = false;
  }
  return o + "},\n";
}
// the "robin" object of a meta.json (either writer's layout): every side it names, two quoted hex floats each
void read_robin(const std::string& js, Meta& m) {
  size_t p = js.find("\"robin\"");
  if (p == std::string::npos) return;
  p = js.find('{', p);
  HEAT2D_REQUIRE(p != std::string::npos, "malformed meta.json: \"robin\" is no object");
  const size_t end = js.find('}', p);
  HEAT2D_REQUIRE(end != std::string::npos, "malformed meta.json: \"robin\" is not closed");
  const std::string obj = js.substr(p, end - p);
  for (int k = 0; k < 4; ++k) {
    size_t q = obj.find(std::string("\"") + kRobinKeys[k] + "\"");
    if (q == std::string::npos) continue;
    q = obj.find('[', q);
    HEAT2D_REQUIRE(q != std::string::npos, "malformed meta.json: a Robin side is no pair");
    for (int v = 0; v < 2; ++v) {
      const size_t a = obj.find('"', q + 1);
      const size_t b = a == std::string::npos ? a : obj.find('"', a + 1);
      HEAT2D_REQUIRE(b != std::string::npos, "malformed meta.json: a Robin side is no pair of strings");
      const std::string t = obj.substr(a + 1, b - a - 1);
      char* e = nullptr;
      m.robin[2 * k + v] = std::strtod(t.c_str(), &e);
      HEAT2D_REQUIRE(e && e != t.c_str() && *e == '\0', "malformed meta.json: a Robin value is no number (" + t + ")");
      q = b;
    }
    m.robin_sides |= 1 << k;
  }
}
// " \"weights\": [\"0x1.cp-4\", ...],\n" ("" without weights)
std::string weights_json(const Meta& m) {
  if (!m.weights_set) return "";
  std::string o = " \"weights\": [";
  for (int i = 0; i < 5; ++i) {
    char b[64];
    std::snprintf(b, sizeof(b), "%s\"%a\"", i ? ", " : "", m.weights[i]);
    o += b;
  }
  return o + "],\n";
}
// the "weights" list of a meta.json (either writer's layout): five quoted hex floats
void read_weights(const std::string& js, Meta& m) {
  size_t p = js.find("\"weights\"");
  if (p == std::string::npos) return;
  size_t q = js.find('[', p);
  HEAT2D_REQUIRE(q != std::string::npos, "malformed meta.json: \"weights\" is no list");
  const size_t end = js.find(']', q);
  HEAT2D_REQUIRE(end != std::string::npos, "malformed meta.json: \"weights\" is not closed");
  for (int i = 0; i < 5; ++i) {
    const size_t a = js.find('"', q + 1);
    const size_t b = a == std::string::npos ? a : js.find('"', a + 1);
    HEAT2D_REQUIRE(b != std::string::npos && b < end, "malformed meta.json: \"weights\" holds fewer than five strings");
    const std::string t = js.substr(a + 1, b - a - 1);
    char* e = nullptr;
    m.weights[i] = std::strtod(t.c_str(), &e);
    HEAT2D_REQUIRE(e && e != t.c_str() && *e == '\0', "malformed meta.json: a weight is no number (" + t + ")");
    q = b;
  }
  m.weights_set = true;
}
}  // namespace

void write_meta(const std::string& dir, const std::string& name, const Meta& m) {
  char buf[2048];
  std::snprintf(buf, sizeof(buf),
                "{\n \"format\": \"%s\",\n \"step\": %lld,\n \"nranks\": %d,\n \"dtype\": \"%s\",\n"
                " \"n_owned\": %lld,\n \"n_input\": %lld,\n \"convention\": \"%s\",\n \"sigma\": %.17g,\n"
                " \"nu\": %.17g,\n \"dom_len\": %.17g,\n \"r\": %.17g,\n \"edge_shift\": %lld,\n"
                " \"bc_x\": \"%s\",\n \"bc_y\": \"%s\",\n \"source_sha256\": %s,\n%s"
                " \"writer\": \"heat2d-cli\"\n}\n",
                kFormat, (long long)m.step, m.nranks, m.dtype == 0 ? "fp32" : "fp64", (long long)m.n_owned,
                (long long)m.n_input, m.convention.c_str(), m.sigma, m.nu, m.dom_len, m.r, (long long)m.edge_shift,
                m.bc_x.c_str(), m.bc_y.c_str(),
                m.source_sha256.empty() ? "null" : ("\"" + m.source_sha256 + "\"").c_str(),
                // (the key only with a diffusivity map: saves without one keep their key set)
                ((m.rmap_sha256.empty() ? "" : " \"rmap_sha256\": \"" + m.rmap_sha256 + "\",\n") +
                 // (and the key of the face coefficients only with them)
                 (m.faces_sha256.empty() ? "" : " \"faces_sha256\": \"" + m.faces_sha256 + "\",\n") +
                 // (and the key of the source's gain schedule only with one)
                 (m.source_gain_sha256.empty() ? "" : " \"source_gain_sha256\": \"" + m.source_gain_sha256 + "\",\n") +
                 // (and the key of the Robin walls' pairs only with a Robin axis)
                 robin_json(m) +
                 // (and the key of the five weights only with them)
                 weights_json(m)).c_str());
  write_atomic(join(join(dir, name), "meta.json"), buf);  // + fsync of the step directory (rank files' entries)
  write_atomic(join(dir, "latest"), name + "\n");  // the commit point
  // prune: keep the two newest complete saves, ordered by (step, generation)
  std::vector<std::string> steps;
  if (DIR* d = ::opendir(dir.c_str())) {
    long long st = 0, g = 0;
    while (dirent* e = ::readdir(d))
      if (step_key(e->d_name, &st, &g)) steps.push_back(e->d_name);
    ::closedir(d);
  }
  std::sort(steps.begin(), steps.end(), [](const std::string& a, const std::string& b) {
    long long sa = 0, ga = 0, sb = 0, gb = 0;
    step_key(a, &sa, &ga);
    step_key(b, &sb, &gb);
    return sa != sb ? sa < sb : ga < gb;
  });
  const auto cur = std::find(steps.begin(), steps.end(), name);
  for (auto it = steps.begin(); cur != steps.end() && it + 1 < cur; ++it) {
    const std::string sd = join(dir, *it);
    if (DIR* d = ::opendir(sd.c_str())) {
      while (dirent* e = ::readdir(d))
        if (e->d_name[0] != '.') ::unlink(join(sd, e->d_name).c_str());
      ::closedir(d);
    }
    ::rmdir(sd.c_str());
  }
}

Meta read_meta(const std::string& dir) {
  std::string sd = dir;
  if (exists(join(dir, "latest"))) {
    std::string name = read_text(join(dir, "latest"));
    while (!name.empty() && (name.back() == '\n' || name.back() == ' ')) name.pop_back();
    sd = join(dir, name);
  }
  HEAT2D_REQUIRE(exists(join(sd, "meta.json")), dir + ": no checkpoint (neither latest nor meta.json)");
  const std::string js = read_text(join(sd, "meta.json"));
  const std::string fmt = json_value(js, "format");
  HEAT2D_REQUIRE(fmt == kFormat || fmt == kFormatV1, dir + ": not a heat2d checkpoint (" + fmt + ")");
  Meta m;
  m.dir = sd;
  m.step = std::atoll(json_value(js, "step").c_str());
  m.nranks = std::atoi(json_value(js, "nranks").c_str());
  m.dtype = json_value(js, "dtype") == "fp32" ? 0 : 1;
  m.n_owned = std::atoll(json_value(js, "n_owned").c_str());
  m.n_input = std::atoll(json_value(js, "n_input").c_str());
  m.convention = json_value(js, "convention");
  m.sigma = std::atof(json_value(js, "sigma").c_str());
  m.nu = std::atof(json_value(js, "nu").c_str());
  m.dom_len = std::atof(json_value(js, "dom_len").c_str());
  m.r = std::atof(json_value(js, "r").c_str());
  if (js.find("\"edge_shift\"") != std::string::npos) m.edge_shift = std::atoll(json_value(js, "edge_shift").c_str());
  if (js.find("\"bc_x\"") != std::string::npos) m.bc_x = json_value(js, "bc_x");
  if (js.find("\"bc_y\"") != std::string::npos) m.bc_y = json_value(js, "bc_y");
  if (js.find("\"source_sha256\"") != std::string::npos) {
    m.source_sha256 = json_value(js, "source_sha256");
    while (!m.source_sha256.empty() && (m.source_sha256.back() == ' ' || m.source_sha256.back() == '\r')) m.source_sha256.pop_back();
    if (m.source_sha256 == "null") m.source_sha256.clear();
  }
  if (js.find("\"rmap_sha256\"") != std::string::npos) {
    m.rmap_sha256 = json_value(js, "rmap_sha256");
    while (!m.rmap_sha256.empty() && (m.rmap_sha256.back() == ' ' || m.rmap_sha256.back() == '\r')) m.rmap_sha256.pop_back();
    if (m.rmap_sha256 == "null") m.rmap_sha256.clear();
  }
  if (js.find("\"source_gain_sha256\"") != std::string::npos) {
    m.source_gain_sha256 = json_value(js, "source_gain_sha256");
    while (!m.source_gain_sha256.empty() && (m.source_gain_sha256.back() == ' ' || m.source_gain_sha256.back() == '\r'))
      m.source_gain_sha256.pop_back();
    if (m.source_gain_sha256 == "null") m.source_gain_sha256.clear();
  }
  if (js.find("\"faces_sha256\"") != std::string::npos) {
    m.faces_sha256 = json_value(js, "faces_sha256");
    while (!m.faces_sha256.empty() && (m.faces_sha256.back() == ' ' || m.faces_sha256.back() == '\r')) m.faces_sha256.pop_back();
    if (m.faces_sha256 == "null") m.faces_sha256.clear();
  }
  read_robin(js, m);
  read_weights(js, m);
  auto bc_ok = [](const std::string& v) { return v == "dirichlet" || v == "periodic" || v == "insulated" || v == "robin"; };
  HEAT2D_REQUIRE(bc_ok(m.bc_x) && bc_ok(m.bc_y),
                 dir + ": meta.json: bc_x / bc_y must be dirichlet, periodic, insulated or robin");
  for (int k = 0; k < 4; ++k)
    HEAT2D_REQUIRE((((k < 2 ? m.bc_x : m.bc_y) == "robin") == ((m.robin_sides >> k & 1) != 0)),
                   dir + ": meta.json: \"robin\" must hold a pair exactly for the sides of the robin axes");
  HEAT2D_REQUIRE(m.nranks >= 1 && m.step >= 0 && m.n_owned >= 1, dir + ": inconsistent meta.json");
  return m;
}

std::string sha256_hex(const void* data, size_t bytes) {
  static const uint32_t k[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
      0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
      0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
      0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
      0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
  auto block = [&](const unsigned char* p) {
    uint32_t w[64];
    for (int i = 0; i < 16; ++i)
      w[i] = ((uint32_t)p[4 * i] << 24) | ((uint32_t)p[4 * i + 1] << 16) | ((uint32_t)p[4 * i + 2] << 8) | p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
      const uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + k[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  };
  const unsigned char* p = static_cast<const unsigned char*>(data);
  size_t left = bytes;
  for (; left >= 64; left -= 64, p += 64) block(p);
  unsigned char tail[128] = {0};
  std::memcpy(tail, p, left);
  tail[left] = 0x80;
  const size_t tl = left + 9 <= 64 ? 64 : 128;
  const uint64_t bits = (uint64_t)bytes * 8;
  for (int i = 0; i < 8; ++i) tail[tl - 1 - i] = (unsigned char)(bits >> (8 * i));
  block(tail);
  if (tl == 128) block(tail + 64);
  char out[65];
  for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
  return std::string(out, 64);
}

namespace {
// planes 0: a 2-D rows x cols array; else a 3-D planes x rows x cols one
std::vector<char> read_array(const std::string& path, int64_t planes, int64_t rows, int64_t cols, int dtype,
                             std::string* sha256) {
  File file(path, "rb");
  const NpyInfo info = npy_header(file.f, path);
  if (planes > 0)
    HEAT2D_REQUIRE(info.planes == planes && info.rows == rows && info.cols == cols,
                   path + ": shape (" + (info.planes ? std::to_string(info.planes) + ", " : "") + std::to_string(info.rows) +
                       ", " + std::to_string(info.cols) + "), the face coefficients of this grid are (" +
                       std::to_string(planes) + ", " + std::to_string(rows) + ", " + std::to_string(cols) + ")");
  HEAT2D_REQUIRE(info.planes == planes && info.rows == rows && info.cols == cols,
                 path + ": shape (" + std::to_string(info.rows) + ", " + std::to_string(info.cols) +
                     "), the frame-inclusive grid is (" + std::to_string(rows) + ", " + std::to_string(cols) + ")");
  const size_t n = (size_t)((planes > 0 ? planes : 1) * rows * cols), es_in = info.dtype == 0 ? 4 : 8, es = dtype == 0 ? 4 : 8;
  std::vector<char> raw(n * es_in);
  HEAT2D_REQUIRE(std::fseek(file.f, info.data_off, SEEK_SET) == 0 && std::fread(raw.data(), es_in, n, file.f) == n,
                 path + ": truncated data");
  std::vector<char> out;
  if (info.dtype == dtype) {
    out.swap(raw);
  } else {
    out.resize(n * es);
    if (dtype == 0) {
      const double* in = reinterpret_cast<const double*>(raw.data());
      float* o = reinterpret_cast<float*>(out.data());
      for (size_t i = 0; i < n; ++i) o[i] = (float)in[i];
    } else {
      const float* in = reinterpret_cast<const float*>(raw.data());
      double* o = reinterpret_cast<double*>(out.data());
      for (size_t i = 0; i < n; ++i) o[i] = (double)in[i];
    }
  }
  if (sha256) *sha256 = sha256_hex(out.data(), out.size());
  return out;
}
}  // namespace

std::vector<char> read_source(const std::string& path, int64_t rows, int64_t cols, int dtype, std::string* sha256) {
  return read_array(path, 0, rows, cols, dtype, sha256);
}

std::vector<char> read_faces(const std::string& path, int64_t rows, int64_t cols, int dtype, std::string* sha256) {
  return read_array(path, 2, rows, cols, dtype, sha256);
}

std::vector<char> read_gain(const std::string& path, int dtype, int64_t* len, std::string* sha256) {
  std::vector<double> g;
  {
    File file(path, "rb");
    unsigned char magic[6] = {0};
    const bool npy = std::fread(magic, 1, 6, file.f) == 6 && std::memcmp(magic, "\x93NUMPY", 6) == 0;
    std::rewind(file.f);
    if (npy) {
      unsigned char head[12];
      HEAT2D_REQUIRE(std::fread(head, 1, 10, file.f) == 10, path + ": truncated header");
      size_t hlen = (size_t)head[8] | ((size_t)head[9] << 8);
      if (head[6] != 1) {
        HEAT2D_REQUIRE(std::fread(head + 10, 1, 2, file.f) == 2, path + ": truncated header");
        hlen |= ((size_t)head[10] << 16) | ((size_t)head[11] << 24);
      }
      HEAT2D_REQUIRE(hlen > 0 && hlen < (1u << 20), path + ": bad header length");
      std::string h(hlen, '\0');
      HEAT2D_REQUIRE(std::fread(&h[0], 1, hlen, file.f) == hlen, path + ": truncated header");
      const bool f8 = h.find("'<f8'") != std::string::npos;
      HEAT2D_REQUIRE(f8 || h.find("'<f4'") != std::string::npos, path + ": dtype is not little-endian f4/f8");
      const size_t sp = h.find("'shape':");
      long long n = 0;
      char close = 0;
      HEAT2D_REQUIRE(sp != std::string::npos && std::sscanf(h.c_str() + sp, "'shape': (%lld,%c", &n, &close) == 2 &&
                         close == ')' && n >= 1,
                     path + ": a gain schedule is a non-empty 1-D array");
      g.resize((size_t)n);
      if (f8) {
        HEAT2D_REQUIRE(std::fread(g.data(), 8, (size_t)n, file.f) == (size_t)n, path + ": truncated data");
      } else {
        std::vector<float> raw((size_t)n);
        HEAT2D_REQUIRE(std::fread(raw.data(), 4, (size_t)n, file.f) == (size_t)n, path + ": truncated data");
        for (size_t i = 0; i < raw.size(); ++i) g[i] = (double)raw[i];
      }
    } else {
      char line[512];
      while (std::fgets(line, sizeof(line), file.f)) {
        if (char* c = std::strchr(line, '#')) *c = '\0';
        char* p = line;
        while (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n') ++p;
        if (!*p) continue;
        char* end = nullptr;
        const double v = std::strtod(p, &end);
        HEAT2D_REQUIRE(end != p, path + ": not a number: " + std::string(p));
        while (*end == ' ' || *end == '\t' || *end == '\r' || *end == '\n') ++end;
        HEAT2D_REQUIRE(!*end, path + ": one number per line");
        g.push_back(v);
      }
      HEAT2D_REQUIRE(!g.empty(), path + ": an empty gain schedule");
    }
  }
  std::vector<char> out(g.size() * (dtype == 0 ? 4 : 8));
  for (size_t i = 0; i < g.size(); ++i) {
    const double v = dtype == 0 ? (double)(float)g[i] : g[i];
    HEAT2D_REQUIRE(std::isfinite(v) && v >= 0.0,
                   path + ": entry " + std::to_string(i) + " is not finite and >= 0 (put the sign into the source)");
    if (dtype == 0) reinterpret_cast<float*>(out.data())[i] = (float)g[i];
    else reinterpret_cast<double*>(out.data())[i] = g[i];
  }
  if (len) *len = (int64_t)g.size();
  if (sha256) *sha256 = sha256_hex(out.data(), out.size());
  return out;
}

void read_rows(const Meta& m, int64_t row0, int64_t nrows, int64_t ncols, int dtype, void* out) {
  HEAT2D_REQUIRE(dtype == m.dtype, "checkpoint dtype differs from the run's --dtype");
  const size_t es = dtype == 0 ? 4 : 8;
  int64_t start = 0;  // global row of the current writer file's first row
  for (int r = 0; r < m.nranks; ++r) {
    const std::string path = rank_file(m.dir, r);
    File file(path, "rb");
    FILE* f = file.f;
    const NpyInfo info = npy_header(f, path);
    HEAT2D_REQUIRE(info.cols == ncols && info.dtype == dtype, path + ": shape / dtype differ from the run");
    HEAT2D_REQUIRE(info.rows == decompose(m.n_owned, m.nranks, r, m.edge_shift).nrows,
                   path + ": row count differs from the writer's decomposition");
    const int64_t a = std::max(row0, start), b = std::min(row0 + nrows, start + info.rows);
    if (a < b) {
      const long off = info.data_off + (long)((a - start) * ncols * (int64_t)es);
      HEAT2D_REQUIRE(std::fseek(f, off, SEEK_SET) == 0, path + ": seek failed");
      const size_t want = (size_t)((b - a) * ncols);
      HEAT2D_REQUIRE(std::fread(static_cast<char*>(out) + (size_t)((a - row0) * ncols) * es, es, want, f) == want,
                     path + ": truncated data");
    }
    start += info.rows;
  }
  HEAT2D_REQUIRE(start == m.n_owned, m.dir + ": rank files do not cover the grid");
}

}  // namespace ckpt
}  // namespace heat2d
