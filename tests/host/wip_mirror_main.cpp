// The two members of bpp::WeightedInnerProductProof (include/bpp_amd.hpp) on the WIP seam: prove a relation over
// PublicKey::new(8) whose statement is trivial (Gc = a, Hc = b, gc = sum a_i b_i y^(i+1) handed in by the caller,
// A' = gamma h), verify it, then tamper.  Compiling and linking is the test on a machine without a GPU.
#include <cstdio>
#include "../../include/bpp_amd.hpp"
using namespace bpp;

int main() {
    Arith::init();
    const size_t len = 8;
    PublicKey pk = PublicKey::create(len);
    // a = b = 0 and y = 2: P = gamma h, and with Gc = Hc = 0, gc = 0 the statement is A' = gamma h
    std::vector<PrimeFieldElem> a(len), b(len), pw(len), zeros(len);
    uint32_t cur = 1;
    for (size_t i = 0; i < len; i++) pw[i] = PrimeFieldElem(cur *= 2);
    const PrimeFieldElem gamma(5);
    WeightedInnerProductProof proof = WeightedInnerProductProof::prove(pk, a, b, pw, gamma, Point::zero());
    MulVec mv;
    mv.add_scalar(gamma);
    mv.add_point(pk.h);
    const Point A_prime = mv.calculate();
    auto ok = proof.verify(pk, pw, zeros, zeros, PrimeFieldElem(0), {}, A_prime, {});
    printf("verify=%s\n", ok ? "Err(VerificationError)" : "Ok(())");
    WeightedInnerProductProof bad = proof;
    bad.d_prime.e[0] ^= 1;
    auto r2 = bad.verify(pk, pw, zeros, zeros, PrimeFieldElem(0), {}, A_prime, {});
    printf("tampered=%s\n", r2 ? "Err(VerificationError)" : "Ok(())");
    return (!ok && r2) ? 0 : 1;
}
