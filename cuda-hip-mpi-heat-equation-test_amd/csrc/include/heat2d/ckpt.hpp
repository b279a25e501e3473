// Native checkpoint / restart (runtime/checkpoint.cpp): the Python driver's
// on-disk format (utils/checkpoint.py), so either driver resumes the other's
// checkpoints on any rank count.
#pragma once

#include <string>
#include <vector>

#include "heat2d/runtime.hpp"

namespace heat2d {
namespace ckpt {

struct Meta {
  int64_t step = 0;
  int nranks = 1;
  int dtype = 1;  // 0 fp32, 1 fp64
  int64_t n_owned = 0, n_input = 0;
  std::string convention = "ghost";  // ghost | inclusive
  double sigma = 0, nu = 0, dom_len = 0, r = 0;
  int64_t edge_shift = 0;  // the writer's decomposition (common.hpp decompose); absent in older saves: 0
  std::string bc_x = "dirichlet", bc_y = "dirichlet";  // dirichlet | periodic | insulated | robin; absent in older saves: dirichlet
  // the Robin walls' pairs in the run's dtype, recorded exactly (meta.json "robin": {side: [a, b]} as hex
  // floats, as utils/checkpoint.py writes them; the key only with a Robin axis). robin_sides: bit k = side
  // k (x_lo, x_hi, y_lo, y_hi) is recorded; robin[2k], robin[2k + 1] its (a, b)
  int robin_sides = 0;
  double robin[8] = {1.0, -0.0, 1.0, -0.0, 1.0, -0.0, 1.0, -0.0};
  // the five weights (wS, wE, wN, wW, wC) in the run's dtype, recorded exactly (meta.json "weights": a list of
  // five hex floats, as utils/checkpoint.py writes it; the key only with weights)
  bool weights_set = false;
  double weights[5] = {};
  // the run's heat source: SHA-256 (hex) of the global frame-inclusive array's bytes in the run's
  // dtype, as utils/checkpoint.py records it; empty: none (null, or absent in older saves)
  std::string source_sha256;
  // the run's diffusivity map, recorded the same way; empty: none (the key is absent)
  std::string rmap_sha256;
  // the run's face coefficients (both arrays, RX then RY), recorded the same way; empty: none (the key is absent)
  std::string faces_sha256;
  // the run's source gain schedule (the converted bytes), recorded the same way; empty: none (the key is absent)
  std::string source_gain_sha256;
  std::string dir;  // read_meta: the directory holding this step's files
};
// A heat source file (--source FILE.npy): a 2-D little-endian f4 / f8 array of exactly rows x cols
// (the frame-inclusive grid; another shape fails), converted to `dtype` (0 fp32, 1 fp64). *sha256
// receives the digest of the converted bytes (Meta::source_sha256).
std::vector<char> read_source(const std::string& path, int64_t rows, int64_t cols, int dtype, std::string* sha256);
// A face-coefficient file (--faces FILE.npy): a 3-D little-endian f4 / f8 array of exactly 2 x rows x cols
// (RX, then RY), converted to `dtype`; *sha256 receives the digest of the converted bytes (Meta::faces_sha256).
std::vector<char> read_faces(const std::string& path, int64_t rows, int64_t cols, int dtype, std::string* sha256);
// A gain schedule file (--source-gain FILE): a 1-D little-endian f4 / f8 .npy, or text with one number
// per line and # comments; non-empty, every entry finite and >= 0, converted to `dtype`. *len receives
// the entry count, *sha256 the digest of the converted bytes (Meta::source_gain_sha256).
std::vector<char> read_gain(const std::string& path, int dtype, int64_t* len, std::string* sha256);
// SHA-256 of a byte range, lower-case hex
std::string sha256_hex(const void* data, size_t bytes);

// Layout (v2): DIR/step-NNNNNNNNNNNN[-G]/{rankNNNNN.npy, meta.json} +
// DIR/latest, a one-line pointer to the newest COMPLETE step directory.
// Collective use: every rank picks the same FRESH step directory
// (step_dir_name, then a barrier before anyone creates it: a step saved again —
// a restart at its final step, a re-run into the same directory — gets a new
// generation -G instead of overwriting files `latest` may point at), writes
// and fsyncs its slab there; after a barrier rank 0 writes meta.json there,
// fsyncs it and the directory, republishes DIR/latest (temp file + fsync +
// rename, atomic) and prunes all but the two newest step directories. A crash
// at any point leaves `latest` on a complete checkpoint; rank files of two
// steps can never be mixed. read_meta also accepts a step directory itself
// and the v1 flat layout (DIR/meta.json + DIR/rank*.npy).
std::string step_dir_name(const std::string& dir, int64_t step);
void write_rank(const std::string& dir, const std::string& name, int rank, Solver& s);
void write_meta(const std::string& dir, const std::string& name, const Meta& m);
Meta read_meta(const std::string& dir);
// Global rows [row0, row0 + nrows) x ncols of the checkpointed field into `out`
// (row-major, ld = ncols), gathered from however many writer files there are
// (their shapes checked against the writer's decomposition).
void read_rows(const Meta& m, int64_t row0, int64_t nrows, int64_t ncols, int dtype, void* out);

}  // namespace ckpt
}  // namespace heat2d
