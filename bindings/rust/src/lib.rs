// lib.rs -- the reference crate's public API (gogoex/BulletProofsPlus src/lib.rs:11-13: PublicKey, RangeProof,
// RangeProver) over libbpp_amd.so, plus the README's RangeVerifier (README.md:47-55) and the MulVec seam
// (src/bls12_381/building_block/mulvec.rs:7-53).  Same names, argument meaning and error behaviour as the reference:
// `verify` returns Err(ProofError::VerificationError), `prove` and `MulVec::calculate` panic on bad lengths.
//
// SOURCE ONLY: the image this repository is built in has no Rust toolchain, so this file has never been compiled.
// The `extern "C"` block (ffi.rs) is generated from include/bpp_amd.h and checked against it by
// tests/test_rust_binding.py, which also checks that every ffi function called below exists with the arity used here.
#![allow(non_snake_case)]
pub mod ffi;

use std::os::raw::c_int;
use std::sync::Once;

/// u64 limbs per base-field element of BLS12-381 (the curve the reference's range proof is wired to,
/// src/range/mod.rs:10-15); a wire point is x | y | infinity flag.
pub const L: usize = 6;
pub const PW: usize = 2 * L + 1;

/// reference src/errors.rs:14-50 (only these two are ever produced on this path)
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub enum ProofError {
    VerificationError,
    FormatError,
}

/// reference src/bls12_381/building_block/point/point.rs:12 -- here the canonical affine wire image
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct Point(pub [u64; PW]);
/// reference src/bls12_381/building_block/scalar/prime_field_elem.rs:13-15 -- canonical little-endian limbs
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct PrimeFieldElem(pub [u64; 4]);

impl Point {
    pub fn zero() -> Point {
        let mut w = [0u64; PW];
        w[2 * L] = 1;
        Point(w)
    }
    pub fn is_zero(&self) -> bool {
        self.0[2 * L] != 0
    }
}
impl PrimeFieldElem {
    /// PrimeFieldElem::new(i32) for non-negative values (prime_field_elem.rs:191-195)
    pub fn new(n: u32) -> PrimeFieldElem {
        PrimeFieldElem([n as u64, 0, 0, 0])
    }
}

static INIT: Once = Once::new();
static mut CTX: *mut ffi::BppCtx = std::ptr::null_mut();

/// reference src/bls12_381/building_block/arith.rs:6-19
pub struct Arith;
impl Arith {
    pub fn init() {
        INIT.call_once(|| unsafe {
            let mut c: *mut ffi::BppCtx = std::ptr::null_mut();
            let rc = ffi::bpp_init(ffi::BPP_BLS12_381_G1, 0, &mut c);
            if rc != 0 {
                panic!("bpp_init failed: {}", rc);
            }
            CTX = c;
        });
    }
}
fn ctx() -> *mut ffi::BppCtx {
    Arith::init();
    unsafe { CTX }
}
fn flat_points(ps: &[Point]) -> Vec<u64> {
    ps.iter().flat_map(|p| p.0.iter().cloned()).collect()
}
fn flat_scalars(ss: &[PrimeFieldElem]) -> Vec<u64> {
    ss.iter().flat_map(|s| s.0.iter().cloned()).collect()
}
fn unflat_points(w: &[u64]) -> Vec<Point> {
    w.chunks(PW).map(|c| {
        let mut a = [0u64; PW];
        a.copy_from_slice(c);
        Point(a)
    }).collect()
}

/// reference src/bls12_381/building_block/mulvec.rs:7-53
pub struct MulVec {
    pub scalars: Vec<PrimeFieldElem>,
    pub points: Vec<Point>,
}
impl MulVec {
    pub fn new() -> MulVec {
        MulVec { scalars: vec![], points: vec![] }
    }
    pub fn add_scalar(&mut self, s: &PrimeFieldElem) {
        self.scalars.push(*s);
    }
    pub fn add_scalars(&mut self, ss: &[PrimeFieldElem]) {
        self.scalars.extend_from_slice(ss);
    }
    pub fn add_point(&mut self, p: &Point) {
        self.points.push(*p);
    }
    pub fn add_points(&mut self, ps: &[Point]) {
        self.points.extend_from_slice(ps);
    }
    pub fn calculate(&self) -> Point {
        if self.scalars.len() != self.points.len() {
            panic!("mulvec: lengths of scalars and points must match"); // mulvec.rs:23-25
        }
        let sc = flat_scalars(&self.scalars);
        let pt = flat_points(&self.points);
        let mut out = [0u64; PW];
        let rc = unsafe { ffi::bpp_msm(ctx(), sc.as_ptr(), pt.as_ptr(), self.scalars.len(), out.as_mut_ptr()) };
        assert!(rc == 0, "bpp_msm failed: {}", rc);
        Point(out)
    }
}

/// reference src/publickey.rs:13-52
pub struct PublicKey {
    pub g: Point,
    pub h: Point,
    pub G_vec: Vec<Point>,
    pub H_vec: Vec<Point>,
}
impl PublicKey {
    pub fn new(length: usize) -> PublicKey {
        let mut gh = vec![0u64; 2 * PW];
        let mut gv = vec![0u64; length.max(1) * PW];
        let mut hv = vec![0u64; length.max(1) * PW];
        let rc = unsafe { ffi::bpp_pk_new(ctx(), length, gh.as_mut_ptr(), gv.as_mut_ptr(), hv.as_mut_ptr()) };
        assert!(rc == 0, "bpp_pk_new failed: {}", rc);
        let ghp = unflat_points(&gh);
        PublicKey { g: ghp[0], h: ghp[1], G_vec: unflat_points(&gv[..length * PW]), H_vec: unflat_points(&hv[..length * PW]) }
    }
    /// generators hashed from a label instead of the reference's test generators (bpp_pk_hashed)
    pub fn from_label(length: usize, label: &[u8]) -> PublicKey {
        let mut gh = vec![0u64; 2 * PW];
        let mut gv = vec![0u64; length.max(1) * PW];
        let mut hv = vec![0u64; length.max(1) * PW];
        let rc = unsafe {
            ffi::bpp_pk_hashed(ctx(), label.as_ptr(), label.len(), length, gh.as_mut_ptr(), gv.as_mut_ptr(), hv.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_pk_hashed failed: {}", rc);
        let ghp = unflat_points(&gh);
        PublicKey { g: ghp[0], h: ghp[1], G_vec: unflat_points(&gv[..length * PW]), H_vec: unflat_points(&hv[..length * PW]) }
    }
    /// g * v + h * gamma (publickey.rs:50-52)
    pub fn commitment(&self, v: u64, gamma: &PrimeFieldElem) -> Point {
        let gh = flat_points(&[self.g, self.h]);
        let mut out = [0u64; PW];
        let rc = unsafe { ffi::bpp_commit(ctx(), gh.as_ptr(), v, gamma.0.as_ptr(), out.as_mut_ptr()) };
        assert!(rc == 0, "bpp_commit failed: {}", rc);
        Point(out)
    }
}

/// reference src/range/prover.rs:13-42
pub struct RangeProver {
    pub v_vec: Vec<u64>,
    pub gamma_vec: Vec<PrimeFieldElem>,
    pub commitment_vec: Vec<Point>,
}
impl RangeProver {
    pub fn new() -> RangeProver {
        RangeProver { v_vec: vec![], gamma_vec: vec![], commitment_vec: vec![] }
    }
    pub fn commit(&mut self, pk: &PublicKey, v: u64, gamma: PrimeFieldElem) {
        self.v_vec.push(v);
        self.gamma_vec.push(gamma);
        self.commitment_vec.push(pk.commitment(v, &gamma)); // keeps the `v as i32` truncation of prover.rs:37
    }
    /// `commit` for a whole 64-bit amount: V = v g + gamma h without the `v as i32` of prover.rs:37 (a two-term MulVec) --
    /// the commitment a proof made under BPP_PROVE_AMOUNT64 verifies against
    pub fn commit_amount(&mut self, pk: &PublicKey, v: u64, gamma: PrimeFieldElem) {
        let sc = flat_scalars(&[PrimeFieldElem([v, 0, 0, 0]), gamma]);
        let pts = flat_points(&[pk.g, pk.h]);
        let mut out = [0u64; PW];
        let rc = unsafe { ffi::bpp_msm(ctx(), sc.as_ptr(), pts.as_ptr(), 2, out.as_mut_ptr()) };
        assert!(rc == 0, "bpp_msm failed: {}", rc);
        self.v_vec.push(v);
        self.gamma_vec.push(gamma);
        self.commitment_vec.push(Point(out));
    }
}

/// README.md:47-55 (the reference's code has no such type; `verify` takes the slice, src/range/mod.rs:57-62)
pub struct RangeVerifier {
    pub commitment_vec: Vec<Point>,
}
impl RangeVerifier {
    pub fn new() -> RangeVerifier {
        RangeVerifier { commitment_vec: vec![] }
    }
    pub fn allocate(&mut self, commitment_vec: &[Point]) {
        self.commitment_vec = commitment_vec.to_vec();
    }
}

/// reference src/weighted_inner_product_proof.rs:25-33
pub struct WeightedInnerProductProof {
    pub L_vec: Vec<Point>,
    pub R_vec: Vec<Point>,
    pub A: Point,
    pub B: Point,
    pub r_prime: PrimeFieldElem,
    pub s_prime: PrimeFieldElem,
    pub d_prime: PrimeFieldElem,
}

impl WeightedInnerProductProof {
    /// reference src/weighted_inner_product_proof.rs:36-227, on the engine's WIP seam (include/bpp_amd.h:
    /// bpp_wip_prove_batch).  `power_of_y_vec` must be [y, y^2, .., y^len]; as the reference's verify (:252, :276) the engine
    /// reads its first entry and rebuilds the rest.  `commitment` is dead in the reference (:57, :137-142) and is ignored.
    /// `engine`: a BatchVerifier of this key with n m = len, or None for a small one created for the call.
    pub fn prove(pk: &PublicKey, a_vec: &[PrimeFieldElem], b_vec: &[PrimeFieldElem], power_of_y_vec: &[PrimeFieldElem],
                 gamma: &PrimeFieldElem, commitment: &Point, engine: Option<&BatchVerifier>) -> WeightedInnerProductProof {
        let _ = commitment;
        let len = pk.G_vec.len();
        assert_eq!(pk.H_vec.len(), len);                        // wip.rs:60-67
        assert_eq!(a_vec.len(), len);
        assert_eq!(b_vec.len(), len);
        assert_eq!(power_of_y_vec.len(), len);
        assert!(len.is_power_of_two());
        let k = len.trailing_zeros() as usize;
        let own;
        let eng = match engine {
            Some(e) => e,
            None => {
                own = BatchVerifier::new(pk, len.min(64), len / len.min(64), 4);
                &own
            }
        };
        assert_eq!(1usize << eng.k, len);
        let (a, b) = (flat_scalars(a_vec), flat_scalars(b_vec));
        let mut pts = vec![0u64; (3 + 2 * k) * PW];
        let mut sc = vec![0u64; 12];
        let rc = unsafe {
            ffi::bpp_wip_prove_batch(eng.handle, a.as_ptr(), b.as_ptr(), power_of_y_vec[0].0.as_ptr(), gamma.0.as_ptr(), 1, 0, 0,
                                     std::ptr::null(), std::ptr::null(), 0, std::ptr::null(), pts.as_mut_ptr(),
                                     sc.as_mut_ptr(), std::ptr::null_mut())
        };
        assert!(rc == 0, "bpp_wip_prove_batch failed: {}", rc);
        let p = unflat_points(&pts);
        let s = |i: usize| PrimeFieldElem([sc[4 * i], sc[4 * i + 1], sc[4 * i + 2], sc[4 * i + 3]]);
        WeightedInnerProductProof { A: p[1], B: p[2], L_vec: p[3..3 + k].to_vec(), R_vec: p[3 + k..3 + 2 * k].to_vec(),
                                    r_prime: s(0), s_prime: s(1), d_prime: s(2) }
    }
    /// reference src/weighted_inner_product_proof.rs:238-328; the four `*_exp` arguments are its *_exp_of_commitment
    /// (:238-247).  A length that does not fit is Err(VerificationError), as :335-337, before anything reaches the engine.
    #[allow(clippy::too_many_arguments)]
    pub fn verify(&self, pk: &PublicKey, power_of_y_vec: &[PrimeFieldElem], G_exp: &[PrimeFieldElem], H_exp: &[PrimeFieldElem],
                  g_exp: &PrimeFieldElem, V_exp: &[PrimeFieldElem], A_prime: &Point, V: &[Point],
                  engine: Option<&BatchVerifier>) -> Result<(), ProofError> {
        let len = pk.G_vec.len();
        let k = self.L_vec.len();
        if k >= 32 || len != 1usize << k || self.R_vec.len() != k || pk.H_vec.len() != len || G_exp.len() != len
            || H_exp.len() != len || power_of_y_vec.len() != len || V_exp.len() != V.len() || V.len() > 64 {
            return Err(ProofError::VerificationError);
        }
        let own;
        let eng = match engine {
            Some(e) => e,
            None => {
                own = BatchVerifier::new(pk, len.min(64), len / len.min(64), 4);
                &own
            }
        };
        if 1usize << eng.k != len {
            return Err(ProofError::VerificationError);
        }
        let mut pts = vec![*A_prime, self.A, self.B];
        pts.extend_from_slice(&self.L_vec);
        pts.extend_from_slice(&self.R_vec);
        pts.extend_from_slice(V);
        let pw = flat_points(&pts);
        let sc = flat_scalars(&[self.r_prime, self.s_prime, self.d_prime]);
        let mut stm = Vec::with_capacity(2 * len + 1 + V.len());
        stm.extend_from_slice(G_exp);
        stm.extend_from_slice(H_exp);
        stm.push(*g_exp);
        stm.extend_from_slice(V_exp);
        let stm = flat_scalars(&stm);
        let mut ok = [1u32; 1];
        let rc = unsafe {
            ffi::bpp_wip_verify_batch(eng.handle, pw.as_ptr(), sc.as_ptr(), power_of_y_vec[0].0.as_ptr(), stm.as_ptr(), V.len(), 1,
                                      0, std::ptr::null(), std::ptr::null(), ok.as_mut_ptr(), std::ptr::null_mut(),
                                      std::ptr::null_mut())
        };
        assert!(rc == 0, "bpp_wip_verify_batch failed: {}", rc);
        if ok[0] == 0 { Ok(()) } else { Err(ProofError::VerificationError) }
    }
}

/// reference src/range/mod.rs:25-28
pub struct RangeProof {
    pub A: Point,
    pub proof: WeightedInnerProductProof,
}
impl RangeProof {
    /// reference src/range/mod.rs:31-55
    pub fn prove(pk: &PublicKey, n: usize, prover: &RangeProver) -> RangeProof {
        let m = prover.v_vec.len();
        let mn = n * m;
        assert!(mn.is_power_of_two());                          // wip.rs:67
        assert_eq!(pk.G_vec.len(), mn);                         // range/mod.rs:90-91, :252-253
        assert_eq!(pk.H_vec.len(), mn);
        let k = mn.trailing_zeros() as usize;
        let gh = flat_points(&[pk.g, pk.h]);
        let (gv, hv) = (flat_points(&pk.G_vec), flat_points(&pk.H_vec));
        let gam = flat_scalars(&prover.gamma_vec);
        let cv = flat_points(&prover.commitment_vec);
        let mut pts = vec![0u64; (3 + 2 * k) * PW];
        let mut sc = vec![0u64; 12];
        let rc = unsafe {
            ffi::bpp_range_prove(ctx(), gh.as_ptr(), gv.as_ptr(), hv.as_ptr(), n, m, prover.v_vec.as_ptr(), gam.as_ptr(),
                                 cv.as_ptr(), pts.as_mut_ptr(), sc.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_prove failed: {}", rc);
        let p = unflat_points(&pts);
        let s = |i: usize| PrimeFieldElem([sc[4 * i], sc[4 * i + 1], sc[4 * i + 2], sc[4 * i + 3]]);
        RangeProof {
            A: p[0],
            proof: WeightedInnerProductProof { A: p[1], B: p[2], L_vec: p[3..3 + k].to_vec(), R_vec: p[3 + k..3 + 2 * k].to_vec(),
                                               r_prime: s(0), s_prime: s(1), d_prime: s(2) },
        }
    }
    /// reference src/range/mod.rs:57-78
    pub fn verify(&self, pk: &PublicKey, n: usize, commitment_vec: &[Point]) -> Result<(), ProofError> {
        let k = self.proof.L_vec.len();
        let mut pts = vec![self.A, self.proof.A, self.proof.B];
        pts.extend_from_slice(&self.proof.L_vec);
        pts.extend_from_slice(&self.proof.R_vec);
        let pw = flat_points(&pts);
        let sc = flat_scalars(&[self.proof.r_prime, self.proof.s_prime, self.proof.d_prime]);
        let gh = flat_points(&[pk.g, pk.h]);
        let (gv, hv) = (flat_points(&pk.G_vec), flat_points(&pk.H_vec));
        let cv = flat_points(commitment_vec);
        let rc: c_int = unsafe {
            ffi::bpp_range_verify(ctx(), gh.as_ptr(), gv.as_ptr(), hv.as_ptr(), n, commitment_vec.len(), pw.as_ptr(), k,
                                  sc.as_ptr(), cv.as_ptr())
        };
        match rc {
            0 => Ok(()),
            1 => Err(ProofError::VerificationError),
            2 => Err(ProofError::FormatError),
            e => panic!("bpp_range_verify: {}", e),
        }
    }
    /// the README's calling convention (README.md:55)
    pub fn verify_with(&self, pk: &PublicKey, n: usize, verifier: &RangeVerifier) -> Result<(), ProofError> {
        self.verify(pk, n, &verifier.commitment_vec)
    }
}

/// Not in the reference (it verifies one proof at a time, src/range/mod.rs:57-78): the engine's batch verifier for ONE
/// (public key, n, m) -- window tables of the 2mn + 2 generators in HBM, built once; `verify_batch` then judges any number of
/// proofs per call and returns the reference's verdict for each of them (include/bpp_amd.h: bpp_verifier_create,
/// bpp_range_verify_batch).  `window_bits` = 0 lets the engine choose; 13 needs ~15 GB at (64,16), 17 ~204 GB.
pub struct BatchVerifier {
    handle: *mut ffi::BppVerifier,
    m: usize,
    k: usize,
}
impl BatchVerifier {
    pub fn new(pk: &PublicKey, n: usize, m: usize, window_bits: i32) -> BatchVerifier {
        assert!(pk.G_vec.len() == n * m && pk.H_vec.len() == n * m, "public key of length n*m");
        let gh = flat_points(&[pk.g, pk.h]);
        let (gv, hv) = (flat_points(&pk.G_vec), flat_points(&pk.H_vec));
        let mut h: *mut ffi::BppVerifier = std::ptr::null_mut();
        let rc = unsafe { ffi::bpp_verifier_create(ctx(), gh.as_ptr(), gv.as_ptr(), hv.as_ptr(), n, m, window_bits as c_int, &mut h) };
        assert!(rc == 0, "bpp_verifier_create: {}", rc);
        BatchVerifier { handle: h, m, k: (n * m).trailing_zeros() as usize }
    }
    /// one `Result` per (proof, its commitments), in order: Ok / Err(VerificationError), as RangeProof::verify would return
    pub fn verify_batch(&self, batch: &[(&RangeProof, &[Point])]) -> Vec<Result<(), ProofError>> {
        let mut pts: Vec<Point> = Vec::with_capacity(batch.len() * (3 + 2 * self.k + self.m));
        let mut scs: Vec<PrimeFieldElem> = Vec::with_capacity(batch.len() * 3);
        for (proof, commitment_vec) in batch {
            assert!(proof.proof.L_vec.len() == self.k && commitment_vec.len() == self.m, "proof of another shape");
            pts.extend_from_slice(&[proof.A, proof.proof.A, proof.proof.B]);
            pts.extend_from_slice(&proof.proof.L_vec);
            pts.extend_from_slice(&proof.proof.R_vec);
            pts.extend_from_slice(commitment_vec);
            scs.extend_from_slice(&[proof.proof.r_prime, proof.proof.s_prime, proof.proof.d_prime]);
        }
        let (pw, sw) = (flat_points(&pts), flat_scalars(&scs));
        let mut ok = vec![0u32; batch.len()];
        let rc = unsafe { ffi::bpp_range_verify_batch(self.handle, pw.as_ptr(), sw.as_ptr(), batch.len(), ok.as_mut_ptr()) };
        assert!(rc == 0, "bpp_range_verify_batch: {}", rc);
        ok.iter().map(|&v| if v == 0 { Ok(()) } else { Err(ProofError::VerificationError) }).collect()
    }
    /// RangeProof::prove for a block in which proof i has values[i].len() = m_i values (a power of two <= m), each against the
    /// prefix key PublicKey::new(n m_i) (include/bpp_amd.h: bpp_range_prove_batch_mixed, literal challenges and blinding).
    /// Returns each proof with its commitments.  amount64 = false: the commitments are RangeProver::commit's, with the
    /// `v as i32` of src/range/prover.rs:37; true (BPP_PROVE_AMOUNT64): V = v g + gamma h over the whole u64, so an amount of
    /// 2^31 or more proves and verifies.
    pub fn prove_batch_mixed(&self, values: &[Vec<u64>], gammas: &[Vec<PrimeFieldElem>], amount64: bool) -> Vec<(RangeProof, Vec<Point>)> {
        assert!(values.len() == gammas.len(), "one gamma list per proof");
        let logn = self.k - self.m.trailing_zeros() as usize;
        let (mut vs, mut gs, mut ms, mut npts) = (Vec::<u64>::new(), Vec::<PrimeFieldElem>::new(), Vec::<u32>::new(), 0usize);
        for (v, g) in values.iter().zip(gammas) {
            assert!(v.len() == g.len() && v.len().is_power_of_two() && v.len() <= self.m, "m_i: a power of two <= m, one gamma per value");
            vs.extend_from_slice(v);
            gs.extend_from_slice(g);
            ms.push(v.len() as u32);
            npts += 3 + 2 * (logn + v.len().trailing_zeros() as usize) + v.len();
        }
        let gw = flat_scalars(&gs);
        let mut pts = vec![0u64; npts * PW];
        let mut sc = vec![0u64; values.len() * 12];
        let flags = if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let rc = unsafe {
            ffi::bpp_range_prove_batch_mixed(self.handle, vs.as_ptr(), gw.as_ptr(), ms.as_ptr(), values.len(), flags, std::ptr::null(), 0,
                                             pts.as_mut_ptr(), sc.as_mut_ptr(), std::ptr::null_mut())
        };
        assert!(rc == 0, "bpp_range_prove_batch_mixed: {}", rc);
        let all = unflat_points(&pts);
        let (mut out, mut at) = (Vec::with_capacity(values.len()), 0usize);
        for (i, v) in values.iter().enumerate() {
            let k = logn + v.len().trailing_zeros() as usize;
            let p = &all[at..at + 3 + 2 * k + v.len()];
            let s = |j: usize| PrimeFieldElem([sc[12 * i + 4 * j], sc[12 * i + 4 * j + 1], sc[12 * i + 4 * j + 2], sc[12 * i + 4 * j + 3]]);
            out.push((RangeProof {
                A: p[0],
                proof: WeightedInnerProductProof { A: p[1], B: p[2], L_vec: p[3..3 + k].to_vec(), R_vec: p[3 + k..3 + 2 * k].to_vec(),
                                                   r_prime: s(0), s_prime: s(1), d_prime: s(2) },
            }, p[3 + 2 * k..].to_vec()));
            at += p.len();
        }
        out
    }
    /// RangeProver::commit (src/range/prover.rs:28-42) for a block of values over this engine's g and h, through its
    /// window tables (include/bpp_amd.h: bpp_commit_batch).  amount64 = false keeps the `v as i32` of prover.rs:37, so each
    /// point equals PublicKey::commitment; true (BPP_PROVE_AMOUNT64) commits the whole u64.
    pub fn commit_batch(&self, values: &[u64], gammas: &[PrimeFieldElem], amount64: bool) -> Vec<Point> {
        assert!(values.len() == gammas.len(), "one gamma per value");
        let gw = flat_scalars(gammas);
        let mut out = vec![0u64; values.len() * PW];
        let flags = if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let rc = unsafe { ffi::bpp_commit_batch(self.handle, values.as_ptr(), gw.as_ptr(), values.len(), flags, out.as_mut_ptr()) };
        assert!(rc == 0, "bpp_commit_batch: {}", rc);
        unflat_points(&out)
    }
    /// A batch of mixed aggregation sizes against this verifier's tables (include/bpp_amd.h: bpp_range_verify_batch_mixed):
    /// proof i with m_i = its commitments' count, a power of two <= m.  Each `Result` is
    /// RangeProof::verify(proof_i, PublicKey::new(n m_i), n, V_i) -- the verdict against the PREFIX key of the proof's own
    /// shape.  A proof whose L_vec / R_vec lengths are not log2(n m_i), or whose m_i the verifier does not take, is
    /// Err(VerificationError) without reaching the engine.
    pub fn verify_batch_mixed(&self, batch: &[(&RangeProof, &[Point])]) -> Vec<Result<(), ProofError>> {
        let logn = self.k - self.m.trailing_zeros() as usize;
        let mut out: Vec<Result<(), ProofError>> = vec![Err(ProofError::VerificationError); batch.len()];
        let (mut pts, mut scs, mut ms, mut at) = (Vec::<Point>::new(), Vec::<PrimeFieldElem>::new(), Vec::<u32>::new(), Vec::new());
        for (i, (proof, commitment_vec)) in batch.iter().enumerate() {
            let mi = commitment_vec.len();
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                continue;
            }
            let ki = logn + mi.trailing_zeros() as usize;
            if proof.proof.L_vec.len() != ki || proof.proof.R_vec.len() != ki {
                continue;   // wip.rs:335-337
            }
            pts.extend_from_slice(&[proof.A, proof.proof.A, proof.proof.B]);
            pts.extend_from_slice(&proof.proof.L_vec);
            pts.extend_from_slice(&proof.proof.R_vec);
            pts.extend_from_slice(commitment_vec);
            scs.extend_from_slice(&[proof.proof.r_prime, proof.proof.s_prime, proof.proof.d_prime]);
            ms.push(mi as u32);
            at.push(i);
        }
        if ms.is_empty() {
            return out;
        }
        let (pw, sw) = (flat_points(&pts), flat_scalars(&scs));
        let mut ok = vec![0u32; ms.len()];
        let rc = unsafe {
            ffi::bpp_range_verify_batch_mixed(self.handle, pw.as_ptr(), sw.as_ptr(), ms.as_ptr(), ms.len(), ok.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_verify_batch_mixed: {}", rc);
        for (j, &i) in at.iter().enumerate() {
            out[i] = if ok[j] == 0 { Ok(()) } else { Err(ProofError::VerificationError) };
        }
        out
    }
    /// A block of SERIALIZED proofs of mixed aggregation sizes (include/bpp_amd.h: bpp_range_verify_batch_serialized_mixed):
    /// `proofs` holds the version 1 containers back to back, container i of bpp_proof_bytes(curve, n, ms[i]) bytes, and
    /// `commitments` ms[i] compressed points per proof, both in the order of `ms`.  Each `Result` is
    /// RangeProof::verify(proof_i, PublicKey::new(n ms[i]), n, V_i), or Err(FormatError) for a container, an encoding or a
    /// scalar the decoder rejects.  `ms = None`: the stream is framed first (`proofs_scan`).  Err(FormatError) for the whole
    /// call when the stream cannot be framed, an ms[i] is not taken by this verifier, or the buffers' lengths are not those
    /// `ms` implies: nothing then reaches the engine.
    pub fn verify_serialized_mixed(&self, proofs: &[u8], commitments: &[u8], ms: Option<&[u32]>, transcript: bool)
                                   -> Result<Vec<Result<(), ProofError>>, ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let scanned;
        let ms: &[u32] = match ms {
            Some(ms) => ms,
            None => {
                scanned = proofs_scan(n, proofs)?;
                &scanned
            }
        };
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes) = (0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi) };
            cbytes += mi * cb;
        }
        if pbytes != proofs.len() || cbytes != commitments.len() {
            return Err(ProofError::FormatError);
        }
        if ms.is_empty() {
            return Ok(Vec::new());
        }
        let mut ok = vec![0u32; ms.len()];
        let flags = if transcript { ffi::BPP_SER_TRANSCRIPT } else { 0 };
        let rc = unsafe {
            ffi::bpp_range_verify_batch_serialized_mixed(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(), ms.len(),
                                                         flags, ok.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_verify_batch_serialized_mixed: {}", rc);
        Ok(ok.iter().map(|&v| match v {
            0 => Ok(()),
            2 => Err(ProofError::FormatError),
            _ => Err(ProofError::VerificationError),
        }).collect())
    }
    /// Mask recovery from wire data (include/bpp_amd.h: bpp_range_recover_masks_mixed): Gamma_i = gamma_0 + z^2 gamma_1 + ..
    /// of proof i from its scalar triple, its challenge block (`challenges`: 3 + k_i scalars per proof in the order of `ms`,
    /// or None for the reference's literals) and the blinding key it was made under; `index` names the blinding index of
    /// each proof (None: index_base + i).  For ms[i] = 1 Gamma_i is the output's mask.  NOT a verification; key and index
    /// together are a view key.  Err(FormatError) when an ms[i] is not taken or a length is not what `ms` implies: nothing
    /// then reaches the engine.
    pub fn recover_masks(&self, scalars: &[[PrimeFieldElem; 3]], ms: &[u32], challenges: Option<&[PrimeFieldElem]>,
                         blind_key: &[u8; 32], index_base: u64, index: Option<&[u64]>) -> Result<Vec<PrimeFieldElem>, ProofError> {
        let logn = self.k - self.m.trailing_zeros() as usize;
        let mut nch = 0usize;
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            nch += 3 + logn + mi.trailing_zeros() as usize;
        }
        if scalars.len() != ms.len() || challenges.map_or(false, |c| c.len() != nch) || index.map_or(false, |x| x.len() != ms.len()) {
            return Err(ProofError::FormatError);
        }
        if ms.is_empty() {
            return Ok(Vec::new());
        }
        let flat: Vec<PrimeFieldElem> = scalars.iter().flat_map(|t| t.iter().cloned()).collect();
        let sw = flat_scalars(&flat);
        let cw = challenges.map(flat_scalars);
        let mut out = vec![0u64; ms.len() * 4];
        let rc = unsafe {
            ffi::bpp_range_recover_masks_mixed(self.handle, sw.as_ptr(), ms.as_ptr(), ms.len(),
                                               cw.as_ref().map_or(std::ptr::null(), |c| c.as_ptr()), blind_key.as_ptr(), index_base,
                                               index.map_or(std::ptr::null(), |x| x.as_ptr()), std::ptr::null(), out.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_recover_masks_mixed: {}", rc);
        Ok(out.chunks(4).map(|c| PrimeFieldElem([c[0], c[1], c[2], c[3]])).collect())
    }
    /// Scans a block of serialized proofs (the input of `verify_serialized_mixed`, made under the transcript) for the outputs
    /// of a blinding key (include/bpp_amd.h: bpp_range_scan_serialized_mixed).  `amounts`: one candidate amount per proof,
    /// read for ms[i] = 1 (None: nothing is confirmed); amount64: the proofs commit whole u64 amounts (BPP_PROVE_AMOUNT64).
    /// Per proof (status, Gamma): 0 -- the output opens to (amount, Gamma), it is the key's and Gamma its mask; 1 -- it does
    /// not (Gamma zero); 2 -- FormatError (Gamma zero); 3 (BPP_SCAN_UNCONFIRMED) -- no amount, or ms[i] > 1.  A scan is NOT a
    /// verification: scan what has been verified.  Err(FormatError) as for `verify_serialized_mixed`.
    pub fn scan_serialized_mixed(&self, proofs: &[u8], commitments: &[u8], ms: &[u32], amount64: bool, blind_key: &[u8; 32],
                                 index_base: u64, index: Option<&[u64]>, amounts: Option<&[u64]>)
                                 -> Result<Vec<(u32, PrimeFieldElem)>, ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes) = (0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi) };
            cbytes += mi * cb;
        }
        if pbytes != proofs.len() || cbytes != commitments.len() || index.map_or(false, |x| x.len() != ms.len())
            || amounts.map_or(false, |x| x.len() != ms.len()) {
            return Err(ProofError::FormatError);
        }
        if ms.is_empty() {
            return Ok(Vec::new());
        }
        let flags = ffi::BPP_SER_TRANSCRIPT | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let mut masks = vec![0u64; ms.len() * 4];
        let mut status = vec![0u32; ms.len()];
        let rc = unsafe {
            ffi::bpp_range_scan_serialized_mixed(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(), ms.len(), flags,
                                                 blind_key.as_ptr(), index_base, index.map_or(std::ptr::null(), |x| x.as_ptr()),
                                                 std::ptr::null(), amounts.map_or(std::ptr::null(), |x| x.as_ptr()),
                                                 masks.as_mut_ptr(), status.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_scan_serialized_mixed: {}", rc);
        Ok(status.iter().zip(masks.chunks(4)).map(|(&s, c)| (s, PrimeFieldElem([c[0], c[1], c[2], c[3]]))).collect())
    }
    /// `scan_serialized_mixed` under MANY keys in one call (include/bpp_amd.h: bpp_range_scan_serialized_mixed_keys): the
    /// decode, the membership test, the challenges and the inversions run once, the key-dependent part per (key, proof)
    /// pair.  The blinding index of proof i (index[i], or index_base + i) is shared by all keys; `amounts` is key-major,
    /// keys.len() x ms.len() (None: nothing is confirmed).  Result: one row per key of (status, Gamma) per proof, the
    /// status words of `scan_serialized_mixed`.  Every key is a view key; a scan is NOT a verification.
    pub fn scan_serialized_mixed_keys(&self, proofs: &[u8], commitments: &[u8], ms: &[u32], amount64: bool, keys: &[[u8; 32]],
                                      index_base: u64, index: Option<&[u64]>, amounts: Option<&[u64]>)
                                      -> Result<Vec<Vec<(u32, PrimeFieldElem)>>, ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes) = (0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi) };
            cbytes += mi * cb;
        }
        let pairs = match keys.len().checked_mul(ms.len()) {
            Some(p) if p <= (0x7fff_ffff / 64) => p,
            _ => return Err(ProofError::FormatError),
        };
        if pbytes != proofs.len() || cbytes != commitments.len() || index.map_or(false, |x| x.len() != ms.len())
            || amounts.map_or(false, |x| x.len() != pairs) {
            return Err(ProofError::FormatError);
        }
        if pairs == 0 {
            return Ok(vec![Vec::new(); keys.len()]);
        }
        let flags = ffi::BPP_SER_TRANSCRIPT | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let mut packed: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut masks = vec![0u64; pairs * 4];
        let mut status = vec![0u32; pairs];
        let rc = unsafe {
            ffi::bpp_range_scan_serialized_mixed_keys(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(), ms.len(),
                                                      flags, packed.as_ptr(), keys.len(), index_base,
                                                      index.map_or(std::ptr::null(), |x| x.as_ptr()),
                                                      amounts.map_or(std::ptr::null(), |x| x.as_ptr()), masks.as_mut_ptr(),
                                                      status.as_mut_ptr())
        };
        for b in packed.iter_mut() {
            unsafe { std::ptr::write_volatile(b, 0) };   // the packed copy of the keys made here
        }
        assert!(rc == 0, "bpp_range_scan_serialized_mixed_keys: {}", rc);
        Ok(status.chunks(ms.len()).zip(masks.chunks(4 * ms.len()))
            .map(|(st, mk)| st.iter().zip(mk.chunks(4)).map(|(&s, c)| (s, PrimeFieldElem([c[0], c[1], c[2], c[3]]))).collect())
            .collect())
    }
    /// amount XOR pad(blind_key, index) per amount (include/bpp_amd.h: bpp_amounts_seal): seals amounts, and opens sealed
    /// ones.  The index of amount i is index[i], or index_base + i: the blinding index of the output's proof.
    pub fn seal_amounts(&self, blind_key: &[u8; 32], index_base: u64, index: Option<&[u64]>, amounts: &[u64])
                        -> Result<Vec<u64>, ProofError> {
        if index.map_or(false, |x| x.len() != amounts.len()) || amounts.len() > 0x7fff_ffff / 64 {
            return Err(ProofError::FormatError);
        }
        let mut out = vec![0u64; amounts.len()];
        if amounts.is_empty() {
            return Ok(out);
        }
        let rc = unsafe {
            ffi::bpp_amounts_seal(ctx(), blind_key.as_ptr(), index_base, index.map_or(std::ptr::null(), |x| x.as_ptr()),
                                  amounts.as_ptr(), amounts.len(), out.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_amounts_seal: {}", rc);
        Ok(out)
    }
    /// Verifies a block AND lists the single outputs that belong to `keys`, the front of the two calls run once
    /// (include/bpp_amd.h: bpp_range_verify_find_serialized_mixed_keys).  `amounts`: sealed -- one sealed amount per proof,
    /// shared by all keys; else key-major keys.len() x ms.len() candidates.  Result: (the verdict of every proof, as
    /// `verify_serialized_mixed` under the transcript gives it; the hits (key number, position, amount, mask) in ascending
    /// (key number, position), at most max_hits of them; the number of hits found).  A hit is a VERIFIED single output
    /// whose commitment opens to the amount and the mask recovered under that key.  Every key is a view key.  With no keys
    /// the block is verified all the same.
    pub fn verify_find_serialized_mixed_keys(&self, proofs: &[u8], commitments: &[u8], ms: &[u32], amount64: bool, sealed: bool,
                                             keys: &[[u8; 32]], index_base: u64, index: Option<&[u64]>, amounts: &[u64],
                                             max_hits: usize)
                                             -> Result<(Vec<u32>, Vec<(u32, u32, u64, PrimeFieldElem)>, usize), ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes) = (0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi) };
            cbytes += mi * cb;
        }
        let pairs = match keys.len().checked_mul(ms.len()) {
            Some(p) if p <= (0x7fff_ffff / 64) => p,
            _ => return Err(ProofError::FormatError),
        };
        if pbytes != proofs.len() || cbytes != commitments.len() || index.map_or(false, |x| x.len() != ms.len())
            || amounts.len() != if sealed { ms.len() } else { pairs } {
            return Err(ProofError::FormatError);
        }
        if ms.is_empty() {
            return Ok((Vec::new(), Vec::new(), 0));
        }
        // no keys: the block is verified all the same, and nothing is listed
        let flags = ffi::BPP_SER_TRANSCRIPT | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 }
            | if sealed { ffi::BPP_FIND_AMOUNTS_SEALED } else { 0 };
        let cap = max_hits.min(pairs);
        let mut packed: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut ok = vec![0u32; ms.len()];
        let mut rec = vec![0u32; cap * 12];
        let mut found = 0u32;
        let rc = unsafe {
            ffi::bpp_range_verify_find_serialized_mixed_keys(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(),
                                                             ms.len(), flags, packed.as_ptr(), keys.len(), index_base,
                                                             index.map_or(std::ptr::null(), |x| x.as_ptr()), amounts.as_ptr(),
                                                             ok.as_mut_ptr(), if cap > 0 { rec.as_mut_ptr() } else { std::ptr::null_mut() },
                                                             cap, &mut found)
        };
        for b in packed.iter_mut() {
            unsafe { std::ptr::write_volatile(b, 0) };   // the packed copy of the keys made here
        }
        assert!(rc == 0, "bpp_range_verify_find_serialized_mixed_keys: {}", rc);
        let hits = rec.chunks(12).take((found as usize).min(cap))
            .map(|h| {
                let w = |t: usize| h[4 + 2 * t] as u64 | (h[5 + 2 * t] as u64) << 32;
                (h[0], h[1], h[2] as u64 | (h[3] as u64) << 32, PrimeFieldElem([w(0), w(1), w(2), w(3)]))
            })
            .collect();
        Ok((ok, hits, found as usize))
    }
    /// view_tag(blind_key, index) per output (include/bpp_amd.h: bpp_view_tags): the byte a SENDER attaches to an output
    /// next to its sealed amount.  The index of output i is index[i], or index_base + i.  The tag authenticates nothing.
    pub fn view_tags(&self, blind_key: &[u8; 32], index_base: u64, index: Option<&[u64]>, count: usize)
                     -> Result<Vec<u8>, ProofError> {
        if index.map_or(false, |x| x.len() != count) || count > 0x7fff_ffff / 64 {
            return Err(ProofError::FormatError);
        }
        let mut out = vec![0u8; count];
        if count == 0 {
            return Ok(out);
        }
        let rc = unsafe {
            ffi::bpp_view_tags(ctx(), blind_key.as_ptr(), index_base, index.map_or(std::ptr::null(), |x| x.as_ptr()), count,
                               out.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_view_tags: {}", rc);
        Ok(out)
    }
    /// `verify_find_serialized_mixed_keys` with the outputs' view tags (include/bpp_amd.h:
    /// bpp_range_verify_find_tagged_serialized_mixed_keys): `tags` holds one byte per proof, shared by all keys; a pair
    /// whose tag does not match its key is ruled out after one hash.  Result: the untagged call's three, and the number of
    /// pairs that passed the tag test.
    pub fn verify_find_tagged_serialized_mixed_keys(&self, proofs: &[u8], commitments: &[u8], ms: &[u32], amount64: bool,
                                                    sealed: bool, keys: &[[u8; 32]], index_base: u64, index: Option<&[u64]>,
                                                    amounts: &[u64], tags: &[u8], max_hits: usize)
                                                    -> Result<(Vec<u32>, Vec<(u32, u32, u64, PrimeFieldElem)>, usize, usize), ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes) = (0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi) };
            cbytes += mi * cb;
        }
        let pairs = match keys.len().checked_mul(ms.len()) {
            Some(p) if p <= (0x7fff_ffff / 64) => p,
            _ => return Err(ProofError::FormatError),
        };
        if pbytes != proofs.len() || cbytes != commitments.len() || index.map_or(false, |x| x.len() != ms.len())
            || amounts.len() != if sealed { ms.len() } else { pairs } || tags.len() != ms.len() {
            return Err(ProofError::FormatError);
        }
        if ms.is_empty() {
            return Ok((Vec::new(), Vec::new(), 0, 0));
        }
        let flags = ffi::BPP_SER_TRANSCRIPT | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 }
            | if sealed { ffi::BPP_FIND_AMOUNTS_SEALED } else { 0 };
        let cap = max_hits.min(pairs);
        let mut packed: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut ok = vec![0u32; ms.len()];
        let mut rec = vec![0u32; cap * 12];
        let (mut found, mut candidates) = (0u32, 0u32);
        let rc = unsafe {
            ffi::bpp_range_verify_find_tagged_serialized_mixed_keys(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(),
                                                                    ms.len(), flags, packed.as_ptr(), keys.len(), index_base,
                                                                    index.map_or(std::ptr::null(), |x| x.as_ptr()), amounts.as_ptr(),
                                                                    ok.as_mut_ptr(), if cap > 0 { rec.as_mut_ptr() } else { std::ptr::null_mut() },
                                                                    cap, &mut found, tags.as_ptr(), &mut candidates)
        };
        for b in packed.iter_mut() {
            unsafe { std::ptr::write_volatile(b, 0) };   // the packed copy of the keys made here
        }
        assert!(rc == 0, "bpp_range_verify_find_tagged_serialized_mixed_keys: {}", rc);
        let hits = rec.chunks(12).take((found as usize).min(cap))
            .map(|h| {
                let w = |t: usize| h[4 + 2 * t] as u64 | (h[5 + 2 * t] as u64) << 32;
                (h[0], h[1], h[2] as u64 | (h[3] as u64) << 32, PrimeFieldElem([w(0), w(1), w(2), w(3)]))
            })
            .collect();
        Ok((ok, hits, found as usize, candidates as usize))
    }
    /// The sender's side of outputs with derived masks (include/bpp_amd.h: bpp_outputs_make): one recipient key and one
    /// amount per OUTPUT, ms[i] outputs in proof i, whose blinding index is index[i] or index_base + i.  Result: the masks
    /// (the gamma of the commit and prove calls; secret), the sealed amounts and the tags, one per output.
    pub fn make_outputs(&self, keys: &[[u8; 32]], amounts: &[u64], ms: &[u32], index_base: u64, index: Option<&[u64]>)
                        -> Result<(Vec<PrimeFieldElem>, Vec<u64>, Vec<u8>), ProofError> {
        let n_out: usize = ms.iter().map(|&m| m as usize).sum();
        if keys.len() != n_out || amounts.len() != n_out || index.map_or(false, |x| x.len() != ms.len())
            || n_out > 0x7fff_ffff / 64 {
            return Err(ProofError::FormatError);
        }
        if n_out == 0 {
            return Ok((Vec::new(), Vec::new(), Vec::new()));
        }
        let (mut idx, mut place) = (Vec::with_capacity(n_out), Vec::with_capacity(n_out));
        for (i, &m) in ms.iter().enumerate() {
            for j in 0..m {
                idx.push(index.map_or(index_base.wrapping_add(i as u64), |x| x[i]));
                place.push(j);
            }
        }
        let mut packed: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut masks = vec![0u64; n_out * 4];
        let mut sealed = vec![0u64; n_out];
        let mut tags = vec![0u8; n_out];
        let rc = unsafe {
            ffi::bpp_outputs_make(ctx(), packed.as_ptr(), idx.as_ptr(), place.as_ptr(), amounts.as_ptr(), n_out, masks.as_mut_ptr(),
                                  sealed.as_mut_ptr(), tags.as_mut_ptr())
        };
        for b in packed.iter_mut() {
            unsafe { std::ptr::write_volatile(b, 0) };   // the packed copy of the keys made here
        }
        assert!(rc == 0, "bpp_outputs_make: {}", rc);
        Ok((masks.chunks(4).map(|w| PrimeFieldElem([w[0], w[1], w[2], w[3]])).collect(), sealed, tags))
    }
    /// Verifies a block and lists, per OUTPUT, what belongs to the keys, aggregated proofs included (include/bpp_amd.h:
    /// bpp_range_verify_find_outputs_serialized_mixed_keys): `sealed` and `tags` hold one entry per output (the sum of
    /// `ms`), in caller order, shared by all keys.  Result: the verdicts, the hits as (key number, output number, amount,
    /// mask), the hits found and the pairs that passed the tag test.
    pub fn verify_find_outputs_serialized_mixed_keys(&self, proofs: &[u8], commitments: &[u8], ms: &[u32], amount64: bool,
                                                     keys: &[[u8; 32]], index_base: u64, index: Option<&[u64]>, sealed: &[u64],
                                                     tags: &[u8], max_hits: usize)
                                                     -> Result<(Vec<u32>, Vec<(u32, u32, u64, PrimeFieldElem)>, usize, usize), ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes, mut n_out) = (0usize, 0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi) };
            cbytes += mi * cb;
            n_out += mi;
        }
        let pairs = match keys.len().checked_mul(n_out) {
            Some(p) if p <= (0x7fff_ffff / 64) => p,
            _ => return Err(ProofError::FormatError),
        };
        if pbytes != proofs.len() || cbytes != commitments.len() || index.map_or(false, |x| x.len() != ms.len())
            || sealed.len() != n_out || tags.len() != n_out {
            return Err(ProofError::FormatError);
        }
        if ms.is_empty() {
            return Ok((Vec::new(), Vec::new(), 0, 0));
        }
        let flags = ffi::BPP_SER_TRANSCRIPT | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let cap = max_hits.min(pairs);
        let mut packed: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut ok = vec![0u32; ms.len()];
        let mut rec = vec![0u32; cap * 12];
        let (mut found, mut candidates) = (0u32, 0u32);
        let rc = unsafe {
            ffi::bpp_range_verify_find_outputs_serialized_mixed_keys(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(),
                                                                     ms.len(), flags, packed.as_ptr(), keys.len(), index_base,
                                                                     index.map_or(std::ptr::null(), |x| x.as_ptr()), sealed.as_ptr(),
                                                                     tags.as_ptr(), ok.as_mut_ptr(),
                                                                     if cap > 0 { rec.as_mut_ptr() } else { std::ptr::null_mut() },
                                                                     cap, &mut found, &mut candidates)
        };
        for b in packed.iter_mut() {
            unsafe { std::ptr::write_volatile(b, 0) };   // the packed copy of the keys made here
        }
        assert!(rc == 0, "bpp_range_verify_find_outputs_serialized_mixed_keys: {}", rc);
        let hits = rec.chunks(12).take((found as usize).min(cap))
            .map(|h| {
                let w = |t: usize| h[4 + 2 * t] as u64 | (h[5 + 2 * t] as u64) << 32;
                (h[0], h[1], h[2] as u64 | (h[3] as u64) << 32, PrimeFieldElem([w(0), w(1), w(2), w(3)]))
            })
            .collect();
        Ok((ok, hits, found as usize, candidates as usize))
    }

    /// The byte counts of a ragged block (include/bpp_amd.h: "proofs over ANY number of outputs"): proof i covers outs[i]
    /// outputs, 1 <= outs[i] <= m, has the container of shape (n, 2^ceil(log2 outs[i])) and outs[i] encoded commitments.
    /// -> (container bytes, commitment bytes, outputs); Err(FormatError) for a count that is not taken.
    fn outs_bytes(&self, outs: &[u32]) -> Result<(usize, usize, usize), ProofError> {
        let n = 1usize << (self.k - self.m.trailing_zeros() as usize);
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let ms = outs_shapes(outs, self.m)?;
        let (mut pbytes, mut n_out) = (0usize, 0usize);
        for (&mi, &o) in ms.iter().zip(outs) {
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, mi as usize) };
            n_out += o as usize;
        }
        Ok((pbytes, n_out * cb, n_out))
    }
    /// Proves a block whose proofs cover ANY number of outputs (include/bpp_amd.h: bpp_range_prove_batch_serialized_outs):
    /// values[i], gammas[i] hold the 1..m values and masks of proof i, which is the proof of shape (n, 2^ceil(log2 len))
    /// over them padded with zeros.  -> (containers back to back, outs[i] encoded commitments per proof back to back, outs).
    pub fn prove_serialized_outputs(&self, values: &[Vec<u64>], gammas: &[Vec<PrimeFieldElem>], transcript: bool, amount64: bool)
                                    -> Result<(Vec<u8>, Vec<u8>, Vec<u32>), ProofError> {
        if values.len() != gammas.len() || values.iter().zip(gammas).any(|(v, g)| v.len() != g.len()) {
            return Err(ProofError::FormatError);
        }
        let outs: Vec<u32> = values.iter().map(|v| v.len() as u32).collect();
        let (pbytes, cbytes, _) = self.outs_bytes(&outs)?;
        if outs.is_empty() {
            return Ok((Vec::new(), Vec::new(), outs));
        }
        let vs: Vec<u64> = values.iter().flatten().copied().collect();
        let gs: Vec<PrimeFieldElem> = gammas.iter().flatten().copied().collect();
        let gw = flat_scalars(&gs);
        let (mut proofs, mut commitments) = (vec![0u8; pbytes], vec![0u8; cbytes]);
        let flags = if transcript { ffi::BPP_SER_TRANSCRIPT } else { 0 } | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let rc = unsafe {
            ffi::bpp_range_prove_batch_serialized_outs(self.handle, vs.as_ptr(), gw.as_ptr(), outs.as_ptr(), outs.len(), flags,
                                                       std::ptr::null(), 0, proofs.as_mut_ptr(), commitments.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_prove_batch_serialized_outs: {}", rc);
        Ok((proofs, commitments, outs))
    }
    /// Verifies such a block (include/bpp_amd.h: bpp_range_verify_batch_serialized_outs): `commitments` holds outs[i]
    /// encoded points per proof; the padded ones are the identity and are not in the stream.  Err(FormatError) when a
    /// count is not taken or a length is not what `outs` implies: nothing then reaches the engine.
    pub fn verify_serialized_outputs(&self, proofs: &[u8], commitments: &[u8], outs: &[u32], transcript: bool)
                                     -> Result<Vec<Result<(), ProofError>>, ProofError> {
        let (pbytes, cbytes, _) = self.outs_bytes(outs)?;
        if pbytes != proofs.len() || cbytes != commitments.len() {
            return Err(ProofError::FormatError);
        }
        if outs.is_empty() {
            return Ok(Vec::new());
        }
        let mut ok = vec![0u32; outs.len()];
        let flags = if transcript { ffi::BPP_SER_TRANSCRIPT } else { 0 };
        let rc = unsafe {
            ffi::bpp_range_verify_batch_serialized_outs(self.handle, proofs.as_ptr(), commitments.as_ptr(), outs.as_ptr(), outs.len(),
                                                        flags, ok.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_range_verify_batch_serialized_outs: {}", rc);
        Ok(ok.iter().map(|&v| match v {
            0 => Ok(()),
            2 => Err(ProofError::FormatError),
            _ => Err(ProofError::VerificationError),
        }).collect())
    }
    /// verify_find_outputs_serialized_mixed_keys over such a block (include/bpp_amd.h:
    /// bpp_range_verify_find_outputs_serialized_outs_keys): `sealed` and `tags` hold one entry per REAL output (the sum of
    /// `outs`), and the output numbers of the hits count real outputs only.
    pub fn verify_find_outputs_serialized_outs_keys(&self, proofs: &[u8], commitments: &[u8], outs: &[u32], amount64: bool,
                                                    keys: &[[u8; 32]], index_base: u64, index: Option<&[u64]>, sealed: &[u64],
                                                    tags: &[u8], max_hits: usize)
                                                    -> Result<(Vec<u32>, Vec<(u32, u32, u64, PrimeFieldElem)>, usize, usize), ProofError> {
        let (pbytes, cbytes, n_out) = self.outs_bytes(outs)?;
        let pairs = match keys.len().checked_mul(n_out) {
            Some(p) if p <= (0x7fff_ffff / 64) => p,
            _ => return Err(ProofError::FormatError),
        };
        if pbytes != proofs.len() || cbytes != commitments.len() || index.map_or(false, |x| x.len() != outs.len())
            || sealed.len() != n_out || tags.len() != n_out {
            return Err(ProofError::FormatError);
        }
        if outs.is_empty() {
            return Ok((Vec::new(), Vec::new(), 0, 0));
        }
        let flags = ffi::BPP_SER_TRANSCRIPT | if amount64 { ffi::BPP_PROVE_AMOUNT64 } else { 0 };
        let cap = max_hits.min(pairs);
        let mut packed: Vec<u8> = keys.iter().flat_map(|k| k.iter().copied()).collect();
        let mut ok = vec![0u32; outs.len()];
        let mut rec = vec![0u32; cap * 12];
        let (mut found, mut candidates) = (0u32, 0u32);
        let rc = unsafe {
            ffi::bpp_range_verify_find_outputs_serialized_outs_keys(self.handle, proofs.as_ptr(), commitments.as_ptr(), outs.as_ptr(),
                                                                    outs.len(), flags, packed.as_ptr(), keys.len(), index_base,
                                                                    index.map_or(std::ptr::null(), |x| x.as_ptr()), sealed.as_ptr(),
                                                                    tags.as_ptr(), ok.as_mut_ptr(),
                                                                    if cap > 0 { rec.as_mut_ptr() } else { std::ptr::null_mut() },
                                                                    cap, &mut found, &mut candidates)
        };
        for b in packed.iter_mut() {
            unsafe { std::ptr::write_volatile(b, 0) };   // the packed copy of the keys made here
        }
        assert!(rc == 0, "bpp_range_verify_find_outputs_serialized_outs_keys: {}", rc);
        let hits = rec.chunks(12).take((found as usize).min(cap))
            .map(|h| {
                let w = |t: usize| h[4 + 2 * t] as u64 | (h[5 + 2 * t] as u64) << 32;
                (h[0], h[1], h[2] as u64 | (h[3] as u64) << 32, PrimeFieldElem([w(0), w(1), w(2), w(3)]))
            })
            .collect();
        Ok((ok, hits, found as usize, candidates as usize))
    }
}

/// The aggregation sizes of proofs over `outs[i]` outputs for an engine of capacity `m` (include/bpp_amd.h:
/// bpp_outs_shapes): 2^ceil(log2 outs[i]).  Err(FormatError) for a count of zero or above `m`.  Host code, no device.
pub fn outs_shapes(outs: &[u32], m: usize) -> Result<Vec<u32>, ProofError> {
    let mut ms = vec![0u32; outs.len()];
    let rc = unsafe { ffi::bpp_outs_shapes(outs.as_ptr(), outs.len(), m, ms.as_mut_ptr()) };
    if rc != 0 {
        return Err(ProofError::FormatError);
    }
    Ok(ms)
}

/// The cuts of a batch over `world` shards (include/bpp_amd.h: bpp_shard_cuts): shard r takes proofs
/// [cuts[r], cuts[r + 1]).  `ms = None`: a uniform batch of `count` proofs; else proof i costs ms[i] (and `count` must be
/// ms.len()).  Host code, no device.
pub fn shard_cuts(ms: Option<&[u32]>, count: usize, world: usize) -> Result<Vec<usize>, ProofError> {
    if world == 0 || world > 16 || ms.map_or(false, |m| m.len() != count) {
        return Err(ProofError::FormatError);
    }
    let mut cuts = vec![0usize; world + 1];
    let rc = unsafe { ffi::bpp_shard_cuts(ms.map_or(std::ptr::null(), |m| m.as_ptr()), count, world, cuts.as_mut_ptr()) };
    if rc != 0 {
        return Err(ProofError::FormatError);
    }
    Ok(cuts)
}

/// How `VerifierPool::verify_serialized_mixed` checks a block.
pub enum PoolMode<'a> {
    /// every shard runs the exact per-proof pass over its slice
    Exact,
    /// every shard runs the grouped check over its slice: 32 secret bytes from the OS CSPRNG, the GLOBAL index of the
    /// block's first proof, and the group size (a power of two >= 2)
    Grouped { weight_key: &'a [u8; 32], index_base: u64, group: u32 },
}

/// ONE batch sharded over several devices of a node in this process (include/bpp_amd.h "verifier pool"): per entry of
/// `devices` a context and a verifier of capacity (n, m) on that device; a verify call cuts the batch (shard_cuts), runs
/// the shards' passes on one host thread each and returns the verdicts in caller order.  An ordinal may repeat: the
/// shards then share a device.  One host thread at a time (hence `&mut self`).
pub struct VerifierPool {
    handle: *mut std::os::raw::c_void,
    n: usize,
    m: usize,
    k: usize,
}
impl VerifierPool {
    pub fn new(pk: &PublicKey, n: usize, m: usize, window_bits: i32, devices: &[i32]) -> VerifierPool {
        assert!(pk.G_vec.len() == n * m && pk.H_vec.len() == n * m, "public key of length n*m");
        assert!(!devices.is_empty() && devices.len() <= 16, "1 to 16 devices");
        let gh = flat_points(&[pk.g, pk.h]);
        let (gv, hv) = (flat_points(&pk.G_vec), flat_points(&pk.H_vec));
        let dev: Vec<c_int> = devices.iter().map(|&d| d as c_int).collect();
        let mut h: *mut std::os::raw::c_void = std::ptr::null_mut();
        let rc = unsafe {
            ffi::bpp_pool_create(ffi::BPP_BLS12_381_G1, dev.as_ptr(), dev.len(), gh.as_ptr(), gv.as_ptr(), hv.as_ptr(), n, m,
                                 window_bits as c_int, &mut h)
        };
        assert!(rc == 0 && !h.is_null(), "bpp_pool_create: {}", rc);
        VerifierPool { handle: h, n, m, k: (n * m).trailing_zeros() as usize }
    }
    pub fn size(&self) -> usize {
        unsafe { ffi::bpp_pool_size(self.handle) }
    }
    /// `BatchVerifier::verify_batch_mixed` over the pool (bpp_pool_verify_mixed): each `Result` is
    /// RangeProof::verify(proof_i, PublicKey::new(n m_i), n, V_i).  A proof whose shape the pool does not take is
    /// Err(VerificationError) without reaching the engine.
    pub fn verify_batch_mixed(&mut self, batch: &[(&RangeProof, &[Point])]) -> Vec<Result<(), ProofError>> {
        let logn = self.k - self.m.trailing_zeros() as usize;
        let mut out: Vec<Result<(), ProofError>> = vec![Err(ProofError::VerificationError); batch.len()];
        let (mut pts, mut scs, mut ms, mut at) = (Vec::<Point>::new(), Vec::<PrimeFieldElem>::new(), Vec::<u32>::new(), Vec::new());
        for (i, (proof, commitment_vec)) in batch.iter().enumerate() {
            let mi = commitment_vec.len();
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                continue;
            }
            let ki = logn + mi.trailing_zeros() as usize;
            if proof.proof.L_vec.len() != ki || proof.proof.R_vec.len() != ki {
                continue;   // wip.rs:335-337
            }
            pts.extend_from_slice(&[proof.A, proof.proof.A, proof.proof.B]);
            pts.extend_from_slice(&proof.proof.L_vec);
            pts.extend_from_slice(&proof.proof.R_vec);
            pts.extend_from_slice(commitment_vec);
            scs.extend_from_slice(&[proof.proof.r_prime, proof.proof.s_prime, proof.proof.d_prime]);
            ms.push(mi as u32);
            at.push(i);
        }
        if ms.is_empty() {
            return out;
        }
        let (pw, sw) = (flat_points(&pts), flat_scalars(&scs));
        let mut ok = vec![0u32; ms.len()];
        let rc = unsafe {
            ffi::bpp_pool_verify_mixed(self.handle, pw.as_ptr(), sw.as_ptr(), ms.as_ptr(), ms.len(), ok.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_pool_verify_mixed: {}", rc);
        for (j, &i) in at.iter().enumerate() {
            out[i] = if ok[j] == 0 { Ok(()) } else { Err(ProofError::VerificationError) };
        }
        out
    }
    /// `BatchVerifier::verify_serialized_mixed` over the pool (bpp_pool_verify_serialized_mixed): a block of version 1
    /// containers and their compressed commitments, `ms = None` framing the stream first.  Err(FormatError) for the whole
    /// call when the stream cannot be framed, an ms[i] is not taken, the buffers' lengths are not those `ms` implies or
    /// the group is not a power of two >= 2: nothing then reaches the engine.  With PoolMode::Grouped the second value is
    /// [groups that failed, proofs re-verified exactly] summed over the shards (it depends on the cut; the statuses do not).
    pub fn verify_serialized_mixed(&mut self, proofs: &[u8], commitments: &[u8], ms: Option<&[u32]>, transcript: bool,
                                   mode: PoolMode) -> Result<(Vec<Result<(), ProofError>>, [u64; 2]), ProofError> {
        let scanned;
        let ms: &[u32] = match ms {
            Some(ms) => ms,
            None => {
                scanned = proofs_scan(self.n, proofs)?;
                &scanned
            }
        };
        let cb = unsafe { ffi::bpp_point_compressed_bytes(ffi::BPP_BLS12_381_G1) };
        let (mut pbytes, mut cbytes) = (0usize, 0usize);
        for &mi in ms {
            let mi = mi as usize;
            if mi == 0 || !mi.is_power_of_two() || mi > self.m {
                return Err(ProofError::FormatError);
            }
            pbytes += unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, self.n, mi) };
            cbytes += mi * cb;
        }
        if pbytes != proofs.len() || cbytes != commitments.len() {
            return Err(ProofError::FormatError);
        }
        let (mode_id, key, index_base, group) = match mode {
            PoolMode::Exact => (ffi::BPP_POOL_EXACT, std::ptr::null(), 0u64, 0u32),
            PoolMode::Grouped { weight_key, index_base, group } => {
                if group < 2 || !group.is_power_of_two() {
                    return Err(ProofError::FormatError);
                }
                (ffi::BPP_POOL_GROUPED, weight_key.as_ptr(), index_base, group)
            }
        };
        let mut stats = [0u64; 2];
        if ms.is_empty() {
            return Ok((Vec::new(), stats));
        }
        let mut ok = vec![0u32; ms.len()];
        let flags = if transcript { ffi::BPP_SER_TRANSCRIPT } else { 0 };
        let rc = unsafe {
            ffi::bpp_pool_verify_serialized_mixed(self.handle, proofs.as_ptr(), commitments.as_ptr(), ms.as_ptr(), ms.len(), flags,
                                                  mode_id, key, index_base, group, ok.as_mut_ptr(), stats.as_mut_ptr())
        };
        assert!(rc == 0, "bpp_pool_verify_serialized_mixed: {}", rc);
        Ok((ok.iter().map(|&v| match v {
            0 => Ok(()),
            2 => Err(ProofError::FormatError),
            _ => Err(ProofError::VerificationError),
        }).collect(), stats))
    }
    /// The combined check of a uniform batch at the capacity shape (bpp_pool_verify_combined): every shard's weighted sum
    /// and ONE reduce on shard 0's device.  Ok(()) iff the batch passes; on Err the caller asks `verify_batch_mixed` which
    /// proofs failed.  `weight_key`: 32 secret bytes from the OS CSPRNG; `index_base`: the global index of the first proof.
    pub fn verify_combined(&mut self, batch: &[(&RangeProof, &[Point])], weight_key: &[u8; 32], index_base: u64)
                           -> Result<(), ProofError> {
        let mut pts: Vec<Point> = Vec::with_capacity(batch.len() * (3 + 2 * self.k + self.m));
        let mut scs: Vec<PrimeFieldElem> = Vec::with_capacity(batch.len() * 3);
        for (proof, commitment_vec) in batch {
            if proof.proof.L_vec.len() != self.k || proof.proof.R_vec.len() != self.k || commitment_vec.len() != self.m {
                return Err(ProofError::VerificationError);   // a proof of another shape fails the batch
            }
            pts.extend_from_slice(&[proof.A, proof.proof.A, proof.proof.B]);
            pts.extend_from_slice(&proof.proof.L_vec);
            pts.extend_from_slice(&proof.proof.R_vec);
            pts.extend_from_slice(commitment_vec);
            scs.extend_from_slice(&[proof.proof.r_prime, proof.proof.s_prime, proof.proof.d_prime]);
        }
        let (pw, sw) = (flat_points(&pts), flat_scalars(&scs));
        let mut ok = 1u32;
        let rc = unsafe {
            ffi::bpp_pool_verify_combined(self.handle, pw.as_ptr(), sw.as_ptr(), batch.len(), weight_key.as_ptr(), index_base, &mut ok)
        };
        assert!(rc == 0, "bpp_pool_verify_combined: {}", rc);
        if ok == 0 { Ok(()) } else { Err(ProofError::VerificationError) }
    }
}
impl Drop for VerifierPool {
    fn drop(&mut self) {
        unsafe { ffi::bpp_pool_destroy(self.handle) }
    }
}

/// m_i of every container of a bare stream of version 1 containers for n-bit values (include/bpp_amd.h: bpp_proofs_scan; host
/// code, no device).  Err(FormatError) when the stream cannot be framed.
pub fn proofs_scan(n: usize, proofs: &[u8]) -> Result<Vec<u32>, ProofError> {
    // the shortest container (m = 1) bounds the count
    let shortest = unsafe { ffi::bpp_proof_bytes(ffi::BPP_BLS12_381_G1, n, 1) };
    if shortest == 0 {
        return Err(ProofError::FormatError);
    }
    let mut ms = vec![0u32; proofs.len() / shortest];
    let mut count = 0usize;
    let rc = unsafe {
        ffi::bpp_proofs_scan(ffi::BPP_BLS12_381_G1, n, 1, proofs.as_ptr(), proofs.len(), ms.as_mut_ptr(), ms.len(), &mut count)
    };
    if rc != 0 {
        return Err(ProofError::FormatError);
    }
    ms.truncate(count);
    Ok(ms)
}
impl Drop for BatchVerifier {
    fn drop(&mut self) {
        unsafe { ffi::bpp_verifier_destroy(self.handle) };
    }
}
