// Stand-alone host program around the flight model's table builder (dev_model.hpp) for tests/test_flight_model_layout_cpu.py:
//   flight_layout_host <fly_flight.ffmb>
// builds the arena, resolves the struct's pointer fields against the host copy (HostModel::fixup, as the backend does against the
// device copy) and prints one line per table:
//   table <name> <lay:: offset> <capacity bytes> <elements> <element size> <mismatches> <bytes behind the capacity that are not zero>
// where a mismatch is an element that reads differently through the struct's pointer field than at arena + offset, and the last column
// looks at the alignment gap up to the next table.  Then `key value` lines.  Built with -fsanitize=address,undefined: a pointer field
// or an offset that leaves the arena ends the program with a report.
#define CVX_HOST 1  // convex.hpp (pulled in by dev_model.hpp) without the HIP runtime
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

struct float4 { float x, y, z, w; };  // the one HIP vector type dev_model.hpp names

#include "../flybody_amd/csrc/dev_model.hpp"

static std::vector<char> slurp(const char *path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("cannot open ") + path);
  return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

template <typename E>
static void table(const char *name, const E *field, size_t off, size_t cap, size_t count, size_t next, const std::vector<unsigned char> &arena) {
  size_t bad = 0, dirty = 0;
  for (size_t k = 0; k < count; k++) {
    E a, b;
    std::memcpy(&a, &field[k], sizeof(E));                       // what the struct's pointer field addresses
    std::memcpy(&b, arena.data() + off + k * sizeof(E), sizeof(E));  // what the kernel reads at the fixed offset
    bad += std::memcmp(&a, &b, sizeof(E)) != 0;
  }
  bad += reinterpret_cast<const unsigned char *>(field) != arena.data() + off;
  for (size_t k = off + cap; k < next && k < arena.size(); k++) dirty += arena[k] != 0;
  std::printf("table %s %zu %zu %zu %zu %zu %zu\n", name, off, cap, count, sizeof(E), bad, dirty);
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s fly_flight.ffmb\n", argv[0]); return 2; }
  using namespace ffe;  // (the table list names the capacities unqualified)
  try {
    const std::vector<char> fb = slurp(argv[1]);
    const ffe::HostModel H = ffe::build_host_model(ffe::Blob(fb.data(), fb.size()));
    ffe::DevModel M;
    H.fixup(M, H.arena.data());
    const size_t nt = ffe::lay::kTables;
    size_t next[nt + 1];
    for (size_t k = 0; k <= nt; k++) next[k] = ffe::lay::start_of((int)k);
#define X(n, t, c) table<t>(#n, M.n, ffe::lay::n, ffe::lay::kBytes[ffe::lay::id_##n], (size_t)(c), next[ffe::lay::id_##n + 1], H.arena);
    FFE_MODEL_TABLES(X)
#undef X
    // the tail: the factorisation schedule with its read-ahead rounds
    const size_t fs_words = (size_t)(M.fs_rounds + 10) * ffe::kWave;
    table<unsigned int>("fsched", M.fsched, ffe::lay::fsched, fs_words * 4, fs_words, ffe::lay::fsched + fs_words * 4, H.arena);
    std::printf("tables %zu\nheader %zu\nstruct_bytes %zu\narena_bytes %zu\nalign %zu\n", nt, ffe::lay::kHeader, sizeof(ffe::DevModel), H.arena.size(), ffe::lay::kAlign);
    std::printf("arena_field %d\n", M.arena == H.arena.data() ? 1 : 0);
    size_t head = 0;
    for (size_t k = 0; k < ffe::lay::kHeader; k++) head += H.arena[k] != 0;
    std::printf("header_nonzero %zu\n", head);  // (the backend writes the resolved struct there after the upload)
    std::printf("nv %d\nnq %d\nnu %d\nnM %d\nnlink %d\nncg %d\nncp %d\nfs_rounds %d\n", M.nv, M.nq, M.nu, M.nM, M.nlink, M.ncg, M.ncp, M.fs_rounds);
    std::printf("solve_dims %u\nnroot %d\nnbr_steps %d\n", M.solve_dims, M.nroot, M.nbr_steps);
    // contents that do not depend on the layout: the tables say what the blob says
    const ffe::Blob blob(fb.data(), fb.size());
    size_t wrong = 0;
    for (int k = 0; k < M.nq; k++) wrong += M.qpos0[k] != static_cast<float>(blob.get("qpos0").f(k));
    for (int k = 0; k < M.nlink; k++) wrong += M.l_parent[k] != blob.get("link_parent").i(k);
    for (int k = 0; k < M.nM; k++) wrong += M.colmadr[k] != M.d_madr[M.m_col[k]] || M.m_row[k] >= M.nv;
    for (int g = 0; g < M.ncg; g++) wrong += M.cg_type[g] != blob.get("geom_type").i(g) || M.cg_link[g] != blob.get("cgeom_link").i(g);
    for (int k = 0; k < ffe::kMaxPair; k++) wrong += (k < M.ncp) != (M.cp_pair[k] != 0xffffu);
    std::printf("content_wrong %zu\n", wrong);
    return 0;
  } catch (const std::exception &e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}
