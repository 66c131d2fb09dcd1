// Evaluates the fc-stack rollout routing (humanoid_mppi-rl_amd/csrc/fc_route.h: fc_route + fc_route_name) on the CPU
// for tests/test_fc_route.py: the nets are packed from blobs by mppi_nets.cpp (host code only: no GPU), the shapes, probe
// outcomes, CU count and knobs come from a rows file, one printed kernel name per row.
//
// usage: fc_route_table <ca blob> <mlp blob> <rows file>
// row:   net(ca|mlp) precision B K Kp H cost_kind nx nu x3_l1 x3_f16 cus  fc_wave x3_wave x3_pair x3d x3h x3h_ns x3m x3m32
//        x3_tiles x3_l1_terms x3_f16_knob x3_f16_l2
#include <cstdio>
#include <fstream>
#include <iterator>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../humanoid_mppi-rl_amd/csrc/fc_route.h"

namespace mppi {
std::vector<unsigned char> build_fc_net(int kind, const void* blob, size_t nbytes, int precision, int nx, int nu,
                                        FcNet& net);
}  // namespace mppi

static std::vector<unsigned char> slurp(const char* path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: fc_route_table ca_blob mlp_blob rows\n");
    return 2;
  }
  const std::vector<unsigned char> blob[2] = {slurp(argv[1]), slurp(argv[2])};
  std::map<std::pair<int, int>, mppi::FcNet> nets;  // (is mlp, precision) -> packed net
  std::ifstream rows(argv[3]);
  std::string line;
  while (std::getline(rows, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string net;
    int precision, cost, nx, nu, x3_l1, x3_f16, cus, x3d, x3h, x3_f16_l2;
    mppi::SolveArgs a{};
    mppi::FcKnobs k;
    in >> net >> precision >> a.B >> a.K >> a.Kp >> a.H >> cost >> nx >> nu >> x3_l1 >> x3_f16 >> cus >> k.fc_wave >> k.x3_wave >>
        k.x3_pair >> x3d >> x3h >> k.x3h_ns >> k.x3m >> k.x3m32 >> k.x3_tiles >> k.x3_l1_terms >> k.x3_f16 >> x3_f16_l2;
    if (!in || (net != "ca" && net != "mlp")) {
      std::fprintf(stderr, "bad row: %s\n", line.c_str());
      return 3;
    }
    k.x3d = x3d != 0;
    k.x3h = x3h != 0;
    k.x3_f16_l2 = x3_f16_l2 != 0;
    a.nx = nx;
    a.nu = nu;
    a.cost_kind = cost;
    const int mlp = net == "mlp";
    auto it = nets.find({mlp, precision});
    if (it == nets.end()) {
      mppi::FcNet n;
      const int kind = mlp ? MPPI_DYN_MLP : MPPI_DYN_CROSS_ATTN;
      mppi::build_fc_net(kind, blob[mlp].data(), blob[mlp].size(), precision, nx, nu, n);
      it = nets.emplace(std::make_pair(mlp, precision), n).first;
    }
    const mppi::FcNet& n = it->second;
    const mppi::FcRoute r = mppi::fc_route(n.arch, n.precision, a, n.fa, x3_l1, x3_f16, cus, k);
    std::printf("%s\n", mppi::fc_route_name(r));
  }
  return 0;
}
