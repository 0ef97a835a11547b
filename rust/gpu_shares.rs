//! Safe adaptor over `hbmpc_sys` (rust/hbmpc_sys.rs, generated from include/hbmpc_hip.h): the reference's own
//! `SecretSharingScheme<Fr>` surface (mpc/src/common/mod.rs:101-128) served by the MI355X library.
//!
//! Where it goes in the reference tree: `mpc/src/gpu/{hbmpc_sys.rs, mod.rs = this file}` behind a cargo feature
//! `gpu`; `build.rs` adds `cargo:rustc-link-search=native=$HBMPC_HIP_LIB_DIR` and `cargo:rustc-link-lib=dylib=hbmpc_hip`.
//! There is no Rust toolchain in the build image of the library, so this file has never met rustc: it is written
//! against the reference's types as they stand (file:line cited at every use) and checked textually against the
//! generated binding (tests/test_rust_shim.py: every `hbmpc_*` call below exists there with that many arguments).
//!
//! * `GpuShares`            one library context; batched calls (`compute_shares_batch`, `batch_recover_secret`, ...)
//! * `GpuRobustShare`       newtype over `RobustShare<Fr>` whose `SecretSharingScheme<Fr>` impl delegates the two
//!                          scheme functions to the process-wide `GpuShares` and every operator to the inner share
//! * `GpuPipeline`          a device-resident pipeline of ALL n simulated parties (`hbmpc_pipe_*`: triple generation,
//!                          fixed-point multiplication, RanSha, RanDouSha, run_preprocessing's triple part) -- what
//!                          `run_preprocessing` (honeybadger/mod.rs:1239-1413), `TripleGenNode::init_batch`
//!                          (triple_gen/triple_generation.rs:304-364) and `FPMulNode::init` (fpmul/fpmul.rs:61-110) drive
//! * `check`                `ShareErrorCode` -> `InterpolateError` / `ShareError`, the inverse of the mapping the
//!                          reference's C bindings apply (mpc/src/ffi/c_bindings/share/mod.rs:18-37)
use std::ffi::{CStr, CString};
use std::ops::{Add, Mul, Sub};
use std::sync::{Mutex, OnceLock};

use ark_bls12_381::Fr;
use ark_ff::{BigInt, PrimeField};
use ark_poly::{univariate::DensePolynomial, DenseUVPolynomial};
use ark_std::rand::Rng;

use super::hbmpc_sys as sys;
use crate::common::share::ShareError; // mpc/src/common/share/mod.rs:12-27
use crate::common::SecretSharingScheme; // mpc/src/common/mod.rs:101-128
use crate::honeybadger::robust_interpolate::robust_interpolate::RobustShare; // robust_interpolate.rs:17-29
use crate::honeybadger::robust_interpolate::InterpolateError; // robust_interpolate/mod.rs:7-27
use crate::honeybadger::fpmul::RandBitError; // fpmul/mod.rs (the error type of fpmul/rand_bit.rs)

// ---- Fr <-> U256: the conversion of mpc/src/ffi/c_bindings/mod.rs:37-49 -------------------------------------------
#[inline]
pub fn to_u256(x: &Fr) -> sys::U256 {
    sys::U256 { data: x.into_bigint().0 }
}
#[inline]
pub fn from_u256(x: &sys::U256) -> Fr {
    // the library only ever returns canonical values (< r), for which from_bigint is Some
    Fr::from_bigint(BigInt::new(x.data)).expect("libhbmpc_hip returned a non-canonical element")
}

/// One library context (one HIP stream).  Calls on one context serialise; create one per worker thread or share it
/// behind the mutex of `global()`.
pub struct GpuShares {
    ctx: *mut sys::HbmpcCtx,
}
// the context is internally locked (include/hbmpc_hip.h: "thread-safe and re-entrant")
unsafe impl Send for GpuShares {}
unsafe impl Sync for GpuShares {}

impl Drop for GpuShares {
    fn drop(&mut self) {
        unsafe { sys::hbmpc_destroy(self.ctx) }
    }
}

impl GpuShares {
    pub fn new(device: i32) -> Result<Self, InterpolateError> {
        let mut ctx: *mut sys::HbmpcCtx = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_create(device, sys::Bls12_381Fr, &mut ctx) };
        if rc != sys::ShareSuccess {
            return Err(InterpolateError::InvalidInput(format!("hbmpc_create(device {device}) -> {rc}: no MI355X available")));
        }
        Ok(GpuShares { ctx })
    }

    fn last_error(&self) -> String {
        let p = unsafe { sys::hbmpc_last_error(self.ctx) };
        if p.is_null() {
            String::new()
        } else {
            unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned()
        }
    }

    /// `ShareErrorCode` -> the error the reference function would have returned.  `n` fills `NoSuitableDomain(n)`.
    fn check(&self, rc: sys::ShareErrorCode, n: usize) -> Result<(), InterpolateError> {
        match rc {
            sys::ShareSuccess => Ok(()),
            sys::InsufficientShares => Err(InterpolateError::ShareError(ShareError::InsufficientShares)),
            sys::DegreeMismatch => Err(InterpolateError::ShareError(ShareError::DegreeMismatch)),
            sys::IdMismatch => Err(InterpolateError::ShareError(ShareError::IdMismatch)),
            sys::TypeMismatch => Err(InterpolateError::ShareError(ShareError::TypeMismatch)),
            sys::InvalidInput => Err(InterpolateError::InvalidInput(self.last_error())),
            sys::NoSuitableDomain => Err(InterpolateError::NoSuitableDomain(n)),
            sys::PolynomialOperationError => Err(InterpolateError::PolynomialOperationError(self.last_error())),
            sys::DecodingError => Err(InterpolateError::DecodingError(self.last_error())),
            other => Err(InterpolateError::InvalidInput(format!("libhbmpc_hip error {other}: {}", self.last_error()))),
        }
    }

    /// `B` calls of `RobustShare::compute_shares` (robust_interpolate.rs:52-82) in one launch.  Draws the rng exactly
    /// like the reference does per secret: `DensePolynomial::rand(degree, rng)`, then `coeffs[0] = secret`.
    /// Returns `[party j][secret b]`.
    pub fn compute_shares_batch(&self, secrets: &[Fr], n: usize, degree: usize, rng: &mut impl Rng)
        -> Result<Vec<Vec<RobustShare<Fr>>>, InterpolateError> {
        let b = secrets.len();
        let mut coeffs = Vec::<sys::U256>::with_capacity(b * (degree + 1));
        for s in secrets {
            let mut poly = DensePolynomial::<Fr>::rand(degree, rng); // same draws, same order (:68)
            poly.coeffs[0] = *s; // (:69)
            coeffs.extend(poly.coeffs.iter().map(to_u256));
        }
        let mut out = vec![sys::U256::default(); n * b];
        let rc = unsafe { sys::hbmpc_compute_shares(self.ctx, coeffs.as_ptr(), b, n, degree, out.as_mut_ptr()) };
        self.check(rc, n)?;
        Ok((0..n)
            .map(|j| out[j * b..(j + 1) * b].iter().map(|v| RobustShare::new(from_u256(v), j, degree)).collect())
            .collect())
    }

    /// Dealer variant with the random coefficients drawn on the device ("hbmpc-chacha20-v1", include/hbmpc_hip.h).
    /// The (seed, index) pair selects the coefficients: NEVER reuse a pair for different secrets -- identical
    /// coefficients would reveal the difference of the secrets to every party.  This adaptor therefore owns the
    /// index: it is a counter of the context that only grows.
    pub fn compute_shares_seeded(&self, secrets: &[Fr], n: usize, degree: usize, seed: &[u8; 32], counter: &mut u64)
        -> Result<Vec<Vec<RobustShare<Fr>>>, InterpolateError> {
        let b = secrets.len();
        let sec: Vec<sys::U256> = secrets.iter().map(to_u256).collect();
        let mut out = vec![sys::U256::default(); n * b];
        let first_index = *counter;
        *counter = counter.checked_add(b as u64).ok_or_else(|| InterpolateError::InvalidInput("seed exhausted".into()))?;
        let rc = unsafe {
            sys::hbmpc_compute_shares_seeded(self.ctx, seed.as_ptr(), sec.as_ptr(), b, first_index, n, degree, out.as_mut_ptr())
        };
        self.check(rc, n)?;
        Ok((0..n)
            .map(|j| out[j * b..(j + 1) * b].iter().map(|v| RobustShare::new(from_u256(v), j, degree)).collect())
            .collect())
    }

    /// `RobustShare::recover_secret` (robust_interpolate.rs:94-157): validation, optimistic interpolation and the
    /// OEC/Gao fallback all happen in the library, in the reference's order and with its error codes.
    pub fn recover_secret(&self, shares: &[RobustShare<Fr>], n: usize, t: usize) -> Result<(Vec<Fr>, Fr), InterpolateError> {
        let s = shares.len();
        let ids: Vec<usize> = shares.iter().map(|x| x.id).collect();
        let degrees: Vec<usize> = shares.iter().map(|x| x.degree).collect();
        let vals: Vec<sys::U256> = shares.iter().map(|x| to_u256(&x.share[0])).collect();
        let cap = shares.first().map_or(1, |x| x.degree + 1);
        let mut coeffs = vec![sys::U256::default(); cap.max(1)];
        let mut ncoeffs: usize = 0;
        let mut secret = sys::U256::default();
        let rc = unsafe {
            sys::hbmpc_recover_secret(self.ctx, ids.as_ptr(), degrees.as_ptr(), vals.as_ptr(), s, n, t, coeffs.as_mut_ptr(),
                                      &mut ncoeffs, &mut secret)
        };
        self.check(rc, n)?;
        Ok((coeffs[..ncoeffs].iter().map(from_u256).collect(), from_u256(&secret)))
    }

    /// `batch_recover_secret` (robust_interpolate.rs:284-443): same arguments, same `Vec<Vec<F>>` (degree + 1
    /// coefficients on the optimistic path, the trimmed vector on the fallback path, the error of the lowest failing
    /// chunk as `Err`).
    pub fn batch_recover_secret(&self, evals_by_sender: &[(usize, Vec<Fr>)], n: usize, degree: usize, t: usize)
        -> Result<Vec<Vec<Fr>>, InterpolateError> {
        let s = evals_by_sender.len();
        let g = evals_by_sender.first().map_or(0, |e| e.1.len());
        if !evals_by_sender.iter().all(|(_, v)| v.len() == g) {
            return Err(InterpolateError::InvalidInput("Inconsistent batch widths".into())); // (:300-306)
        }
        let ids: Vec<usize> = evals_by_sender.iter().map(|(id, _)| *id).collect();
        let flat: Vec<sys::U256> = evals_by_sender.iter().flat_map(|(_, v)| v.iter().map(to_u256)).collect();
        let m = degree + 1;
        let mut coeffs = vec![sys::U256::default(); g * m];
        let mut ncoeffs = vec![0u32; g];
        let rc = unsafe {
            sys::hbmpc_batch_recover(self.ctx, ids.as_ptr(), s, flat.as_ptr(), g, n, degree, t, coeffs.as_mut_ptr(),
                                     ncoeffs.as_mut_ptr(), std::ptr::null_mut())
        };
        self.check(rc, n)?;
        Ok((0..g).map(|c| coeffs[c * m..c * m + ncoeffs[c] as usize].iter().map(from_u256).collect()).collect())
    }

    /// the EvalBatch arm of BatchRecon keeps coefficient 0 only (batch_recon.rs:384-391)
    pub fn batch_recover_p0(&self, evals_by_sender: &[(usize, Vec<Fr>)], n: usize, degree: usize, t: usize)
        -> Result<Vec<Fr>, InterpolateError> {
        let s = evals_by_sender.len();
        let g = evals_by_sender.first().map_or(0, |e| e.1.len());
        if !evals_by_sender.iter().all(|(_, v)| v.len() == g) {
            return Err(InterpolateError::InvalidInput("Inconsistent batch widths".into()));
        }
        let ids: Vec<usize> = evals_by_sender.iter().map(|(id, _)| *id).collect();
        let flat: Vec<sys::U256> = evals_by_sender.iter().flat_map(|(_, v)| v.iter().map(to_u256)).collect();
        let mut secrets = vec![sys::U256::default(); g];
        let rc = unsafe {
            sys::hbmpc_batch_recover_p0(self.ctx, ids.as_ptr(), s, flat.as_ptr(), g, n, degree, t, secrets.as_mut_ptr(),
                                        std::ptr::null_mut())
        };
        self.check(rc, n)?;
        Ok(secrets.iter().map(from_u256).collect())
    }

    /// `make_vandermonde` + `apply_vandermonde` over G chunks (common/share/mod.rs:31-76, batch_recon.rs:157-165):
    /// `chunks[g]` holds d + 1 values; returns `[recipient j][chunk g]`, i.e. row j is the payload for party j.
    pub fn vandermonde_apply(&self, chunks: &[Vec<Fr>], n: usize, degree: usize) -> Result<Vec<Vec<Fr>>, InterpolateError> {
        let g = chunks.len();
        if !chunks.iter().all(|c| c.len() == degree + 1) {
            return Err(InterpolateError::ShareError(ShareError::InvalidInput)); // share/mod.rs:59-64
        }
        let flat: Vec<sys::U256> = chunks.iter().flat_map(|c| c.iter().map(to_u256)).collect();
        let mut out = vec![sys::U256::default(); n * g];
        let rc = unsafe { sys::hbmpc_vandermonde_apply(self.ctx, flat.as_ptr(), g, n, degree, out.as_mut_ptr()) };
        self.check(rc, n)?;
        Ok((0..n).map(|j| out[j * g..(j + 1) * g].iter().map(from_u256).collect()).collect())
    }
}


// ---- device-resident pipelines (include/hbmpc_hip.h, "device-resident pipelines") -------------------------------------
/// One `hbmpc_pipe` handle: the call sequencing, the arena layout and the graph-capture rules live in the library.
/// Buffers are `[party][..]` arrays reached by name (`"a"`, `"b"`, `"r2t"`, `"rt"`, `"c"` for triple generation; see the
/// header for the other kinds).  `run` only enqueues on the handle's stream; `run_checked` reads the decode summaries back
/// and returns the error the reference's `?` would.
pub struct GpuPipeline<'a> {
    gpu: &'a GpuShares,
    pipe: *mut sys::HbmpcPipe,
    owned: bool,
}

impl Drop for GpuPipeline<'_> {
    fn drop(&mut self) {
        if self.owned {
            unsafe { sys::hbmpc_pipe_destroy(self.pipe) }
        }
    }
}

impl GpuShares {
    /// a HIP stream of this context's device for the pipelines (graph capture needs a real stream)
    pub fn stream_create(&self) -> Result<*mut core::ffi::c_void, InterpolateError> {
        let mut s = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_stream_create(self.ctx, &mut s) };
        self.check(rc, 0)?;
        Ok(s)
    }
    /// A host that hands the library buffers from `hipMallocAsync`: the release threshold of the device's stream-ordered pool (0, the
    /// platform default, is the configuration under which such buffers are NOT safe: include/hbmpc_hip.h, "Device buffers") ...
    pub fn stream_pool_release_threshold(&self) -> Result<u64, InterpolateError> {
        let mut thr = 0u64;
        let rc = unsafe { sys::hbmpc_stream_pool_release_threshold(self.ctx, &mut thr) };
        self.check(rc, 0)?;
        Ok(thr)
    }
    /// ... and the one-call remedy: the pool keeps its freed blocks from here on
    pub fn stream_pool_retain(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_stream_pool_retain(self.ctx) };
        self.check(rc, 0)
    }
    fn wrap(&self, rc: sys::ShareErrorCode, pipe: *mut sys::HbmpcPipe, n: usize) -> Result<GpuPipeline<'_>, InterpolateError> {
        self.check(rc, n)?;
        Ok(GpuPipeline { gpu: self, pipe, owned: true })
    }
    // ---- PRandBit / PRandInt (fpmul/prandbitd.rs): device pointers in, device pointers out; `u64` values are folded r_T or Goldilocks elements
    /// the maximal unqualified sets in the order the conversion indexes them: `(0..n).combinations(t)` (prandbitd.rs:479)
    pub fn riss_tsets(n: usize, t: usize) -> Option<Vec<Vec<usize>>> {
        let mut count = 0usize;
        if unsafe { sys::hbmpc_riss_tsets(n, t, std::ptr::null_mut(), &mut count) } != sys::ShareSuccess {
            return None;
        }
        let mut ids = vec![0usize; count * t];
        if unsafe { sys::hbmpc_riss_tsets(n, t, ids.as_mut_ptr(), &mut count) } != sys::ShareSuccess {
            return None;
        }
        Some(if t == 0 { vec![Vec::new(); count] } else { ids.chunks(t).map(|c| c.to_vec()).collect() })
    }
    /// the fold of prandbitd.rs:667-684 with the bound test of :638-647: contrib [n][sets][batch] -> sums [sets][batch], bad [n][sets] bytes
    /// (the caller drops or re-requests the sets with a verdict, where the reference answers `PRandError::InvalidMessage`).
    /// `Err(true)`: `PRandError::SurpassedFieldCapacity` (prandbitd.rs:506-517); `Err(false)`: any other failure (`last_error`)
    #[allow(clippy::too_many_arguments)]
    pub fn riss_fold_dev(&self, contrib: *const u64, n: usize, sets: usize, batch: usize, l_plus_k: usize, sums: *mut u64, bad: *mut u8,
                         stream: *mut core::ffi::c_void) -> Result<(), bool> {
        match unsafe { sys::hbmpc_dev_riss_fold(self.ctx, contrib, n, sets, batch, l_plus_k, sums, bad, stream) } {
            sys::ShareSuccess => Ok(()),
            sys::HBMPC_FIELD_CAPACITY => Err(true),
            _ => Err(false),
        }
    }
    /// the heavy step of `try_advance_from_riss` (prandbitd.rs:311-356) for this node: r over the party's own sets -> its share in this
    /// context's field (`out`: one U256 or one u64 per element) and, when `share_2` is not null, its GF(2^8) share
    #[allow(clippy::too_many_arguments)]
    pub fn riss_convert_own_dev(&self, r: *const u64, n: usize, t: usize, batch: usize, party: usize, out: *mut core::ffi::c_void, share_2: *mut u8,
                                goldilocks: bool, stream: *mut core::ffi::c_void) -> Result<(), InterpolateError> {
        let ids = [party];
        let rc = unsafe {
            if goldilocks {
                sys::hbmpc_gl_dev_riss_convert_parties(self.ctx, r, n, t, batch, ids.as_ptr(), 1, 1, out as *mut u64, share_2, stream)
            } else {
                sys::hbmpc_dev_riss_convert_parties(self.ctx, r, n, t, batch, ids.as_ptr(), 1, 1, out as *mut sys::U256, share_2, stream)
            }
        };
        self.check(rc, n)
    }
    /// the arithmetic of `try_finalize_bit` (prandbitd.rs:189-211) for `parties` parties: b_p = G(v) - r_p, b_2 = r_2 + lsb(v)
    #[allow(clippy::too_many_arguments)]
    pub fn prandbit_finalize_dev(&self, opened: *const u64, r_p: *const sys::U256, r_2: *const u8, batch: usize, parties: usize, b_p: *mut sys::U256,
                                 b_2: *mut u8, stream: *mut core::ffi::c_void) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_dev_prandbit_finalize_parties(self.ctx, opened, r_p, r_2, batch, parties, b_p, b_2, stream) };
        self.check(rc, parties)
    }
    /// `TripleGenNode::init_batch` + BatchRecon(2t) + finalize for all n parties (triple_gen/triple_generation.rs:304-364,164-232)
    pub fn pipe_triplegen(&self, n: usize, t: usize, triples: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_triplegen_create(self.ctx, n, t, triples, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `FPMulNode::init` = Beaver multiplication + TruncPr for all n parties (fpmul/fpmul.rs:61-110, fpmul/truncpr.rs:185-318)
    pub fn pipe_fpmul(&self, n: usize, t: usize, pairs: usize, k: usize, m: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_fpmul_create(self.ctx, n, t, pairs, k, m, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `Multiply::init` for all n parties (honeybadger/mod.rs:543-628, mul/multiplication.rs:417-426,102-139,57-100; `mul_int`, :1177-1223,
    /// wraps it): buffers x, y, ta, tb, tc ([party][pairs]), out = the shares of x * y
    pub fn pipe_mul(&self, n: usize, t: usize, pairs: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_mul_create(self.ctx, n, t, pairs, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// Input for all n parties (honeybadger/input/input.rs:489-506, 85-100, 300-301): buffers x ([values]), r ([party][values], the shares
    /// of the masks); mask, masked ([values]), out = the shares of x.  A mask that does not open refuses its element (zeros, never x + 0)
    pub fn pipe_input(&self, n: usize, t: usize, values: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_input_create(self.ctx, n, t, values, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// Output's client side for all n parties' result shares (honeybadger/output/output.rs:157-177): buffer sh ([party][values]), out ([values])
    pub fn pipe_output(&self, n: usize, t: usize, values: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_output_create(self.ctx, n, t, values, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `BatchReconNode` for all n parties (honeybadger/batch_recon/batch_recon.rs:144-185, 371-391, 451-467): buffer x ([party][values],
    /// values a multiple of degree + 1), Y, Z the two arms' messages, opened ([values]); both arms decode from parties 0 .. degree + t
    pub fn pipe_batchrecon(&self, n: usize, t: usize, degree: usize, values: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_batchrecon_create(self.ctx, n, t, degree, values, 0, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `TruncPrNode` on its own for all n parties (fpmul/truncpr.rs:185-318): buffers a, rint ([party][values]), rbits ([party][m][values])
    pub fn pipe_truncpr(&self, n: usize, t: usize, values: usize, k: usize, m: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_truncpr_create(self.ctx, n, t, values, k, m, 0, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `FPDivConstNode::init` for all n parties (fpdiv/fpdiv_const.rs:61-99): values of `k` bits with `f` fractional bits, each divided by
    /// its public denominator (the integers of `ClearFixedPoint`).  The reciprocals are `fixed_point_reciprocal_scaled`'s
    /// (fpdiv/mod.rs:8-60) and are uploaded as `w`; an invalid divisor is `InvalidInput`, as `FPDivConstError::InvalidDivisor` there
    pub fn pipe_fpdiv_const(&self, n: usize, t: usize, k: usize, f: usize, denominators: &[Fr], stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let d: Vec<sys::U256> = denominators.iter().map(to_u256).collect();
        let mut w = vec![sys::U256::default(); d.len()];
        let rc = unsafe { sys::hbmpc_fixed_point_reciprocal_scaled(d.as_ptr(), d.len(), f, w.as_mut_ptr(), std::ptr::null_mut()) };
        self.check(rc, n)?;
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_truncpr_create(self.ctx, n, t, d.len(), 2 * k, f, 0, 1, stream, &mut p) };
        let pipe = self.wrap(rc, p, n)?;
        let rc = unsafe { sys::hbmpc_pipe_upload(pipe.pipe, GpuPipeline::name("w").as_ptr(), w.as_ptr() as *const core::ffi::c_void, w.len()) };
        self.check(rc, n)?;
        let rc = unsafe { sys::hbmpc_pipe_sync(pipe.pipe) };  // the copy reads `w`
        self.check(rc, n)?;
        Ok(pipe)
    }
    /// `RanShaNode` for all n parties, `batch` elements per dealer (share_gen/share_gen.rs:232-289,401-454,516-530)
    pub fn pipe_ransha(&self, n: usize, t: usize, batch: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_ransha_create(self.ctx, n, t, batch, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `DouShaNode` + `RanDouShaNode` for all n parties (ran_dou_sha/mod.rs:371-449,569-602)
    pub fn pipe_randousha(&self, n: usize, t: usize, batch: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_randousha_create(self.ctx, n, t, batch, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `run_preprocessing`'s triple part: RanSha -> a, b; RanDouSha -> r; TripleGen (honeybadger/mod.rs:1239-1393)
    pub fn pipe_preprocessing(&self, n: usize, t: usize, triples: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_preprocessing_create(self.ctx, n, t, triples, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// `RandBit` for all n parties: Beaver square of a, BatchRecon of a^2, phase 2 (fpmul/rand_bit.rs:242-293,197-220); `bits` a multiple
    /// of t + 1 (rand_bit.rs:253-255); either field, as the context was created
    pub fn pipe_randbit(&self, n: usize, t: usize, bits: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_randbit_create(self.ctx, n, t, bits, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// PRandBit for all n parties (fpmul/prandbitd.rs:638-647,667-684,311-356,437-446,189-211; honeybadger/mod.rs:1951-2150): `self` is the
    /// bls12-381 Fr context, `gl` a Goldilocks context on the same device; `bits` a multiple of t + 1 (prandbitd.rs:472-476).  Buffers
    /// contrib, b_q (inputs, `upload_u64`), sums, r_q, rb, opened (`download_u64`), r_p, b_p (`download`), bad, r_2, b_2, rstatus
    /// (`download_bytes`).  One device call per run: one launch for a small batch
    pub fn pipe_prandbit<'a>(&'a self, gl: &'a GpuShares, n: usize, t: usize, bits: usize, l_plus_k: usize,
                             stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'a>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_prandbit_create(self.ctx, gl.ctx, n, t, bits, l_plus_k, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// PRandInt for all n parties (prandbitd.rs:667-684,311-356): any batch; buffers contrib (input), sums, bad, r_p
    pub fn pipe_prandint(&self, n: usize, t: usize, batch: usize, l_plus_k: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_prandint_create(self.ctx, n, t, batch, l_plus_k, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// FixedPrep for all n parties: run_preprocessing's steps 5 and 6 (honeybadger/mod.rs:1396-1410, 1951-2150) -- one refill of the
    /// r_bits / r_int pools that `mul_fixed` drains (:1031-1045).  `self` is the bls12-381 Fr context, `gl` a Goldilocks context on the same
    /// device; one of `n_prandbit` / `n_prandint` may be 0.  Parts `"ransha"`, `"randousha"`, `"triplegen"`, `"randbit"`, `"prandbit"`,
    /// `"prandint"` (`part`); buffers r_bits, r_int (`download`), r_bits2 (`download_bytes`); `take` / `available` drain the pools
    pub fn pipe_fixedprep<'a>(&'a self, gl: &'a GpuShares, n: usize, t: usize, n_prandbit: usize, n_prandint: usize, l_plus_k: usize,
                              stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'a>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_fixedprep_create(self.ctx, gl.ctx, n, t, n_prandbit, n_prandint, l_plus_k, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    // ---- seeded RISS dealing (contract "hbmpc-riss-chacha20-v1", include/hbmpc_hip.h): ONE seed per sender, and a (seed, domain, index)
    // range is never reused -- take `first_index` from a counter that only grows, as the seeded pipelines do
    /// this node's own contributions from its seed: `out` [sets][batch], row T for the parties outside T.  `Err(true)`:
    /// `PRandError::SurpassedFieldCapacity`
    #[allow(clippy::too_many_arguments)]
    pub fn riss_sample_dev(&self, seed: &[u8; 32], n: usize, t: usize, domain: usize, batch: usize, first_index: u64, l_plus_k: usize, out: *mut u64,
                           stream: *mut core::ffi::c_void) -> Result<(), bool> {
        match unsafe { sys::hbmpc_dev_riss_sample(self.ctx, seed.as_ptr(), n, t, domain, batch, first_index, l_plus_k, out, stream) } {
            sys::ShareSuccess => Ok(()),
            sys::HBMPC_FIELD_CAPACITY => Err(true),
            _ => Err(false),
        }
    }
    /// the host-pointer form: -> [sets][batch]
    pub fn riss_sample(&self, seed: &[u8; 32], n: usize, t: usize, domain: usize, batch: usize, first_index: u64, l_plus_k: usize) -> Result<Vec<u64>, bool> {
        let sets = Self::riss_tsets(n, t).ok_or(false)?.len();
        let mut out = vec![0u64; sets * batch];
        match unsafe { sys::hbmpc_riss_sample(self.ctx, seed.as_ptr(), n, t, domain, batch, first_index, l_plus_k, out.as_mut_ptr()) } {
            sys::ShareSuccess => Ok(out),
            sys::HBMPC_FIELD_CAPACITY => Err(true),
            _ => Err(false),
        }
    }
    /// all n senders' values drawn and folded in registers: `seeds` [n][8] u32 on the device -> `sums` [sets][batch]
    #[allow(clippy::too_many_arguments)]
    pub fn riss_sample_fold_dev(&self, seeds: *const u32, n: usize, t: usize, domain: usize, batch: usize, first_index: u64, l_plus_k: usize,
                                sums: *mut u64, stream: *mut core::ffi::c_void) -> Result<(), bool> {
        match unsafe { sys::hbmpc_dev_riss_sample_fold(self.ctx, seeds, n, t, domain, batch, first_index, l_plus_k, sums, stream) } {
            sys::ShareSuccess => Ok(()),
            sys::HBMPC_FIELD_CAPACITY => Err(true),
            _ => Err(false),
        }
    }
    /// PRandInt for all n parties from the senders' seeds (domain 1): `sums`, `bad` (zeros), `r_p` as `hbmpc_dev_prandint_parties` writes them
    #[allow(clippy::too_many_arguments)]
    pub fn prandint_parties_seeded_dev(&self, seeds: *const u32, first_index: u64, n: usize, t: usize, batch: usize, l_plus_k: usize, sums: *mut u64,
                                       bad: *mut u8, r_p: *mut sys::U256, stream: *mut core::ffi::c_void) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_dev_prandint_parties_seeded(self.ctx, seeds, first_index, n, t, batch, l_plus_k, sums, bad, r_p, stream) };
        self.check(rc, n)
    }
    /// the seeded pipelines: a buffer `seeds` ([n][32] bytes, `upload_bytes`) and no `contrib`; `set_stream_index`; `capture` is refused
    pub fn pipe_prandbit_seeded<'a>(&'a self, gl: &'a GpuShares, n: usize, t: usize, bits: usize, l_plus_k: usize,
                                    stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'a>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_prandbit_create_seeded(self.ctx, gl.ctx, n, t, bits, l_plus_k, 0, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    pub fn pipe_prandint_seeded(&self, n: usize, t: usize, batch: usize, l_plus_k: usize, stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'_>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_prandint_create_seeded(self.ctx, n, t, batch, l_plus_k, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    pub fn pipe_fixedprep_seeded<'a>(&'a self, gl: &'a GpuShares, n: usize, t: usize, n_prandbit: usize, n_prandint: usize, l_plus_k: usize,
                                     stream: *mut core::ffi::c_void) -> Result<GpuPipeline<'a>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_fixedprep_create_seeded(self.ctx, gl.ctx, n, t, n_prandbit, n_prandint, l_plus_k, stream, &mut p) };
        self.wrap(rc, p, n)
    }
    /// hbmpc_dev_take_rows: slices of `[party][len]` pools, regrouped, in one launch (at most 8 slices).  Safety: every pointer of every
    /// slice is a device buffer that holds `rows` rows at its stride
    pub unsafe fn take_rows(&self, slices: &[sys::TakeSlice], rows: usize, stream: *mut core::ffi::c_void) -> Result<(), InterpolateError> {
        let rc = sys::hbmpc_dev_take_rows(self.ctx, slices.as_ptr(), slices.len(), rows, stream);
        self.check(rc, rows)
    }
}

impl<'a> GpuPipeline<'a> {
    fn name(name: &str) -> CString {
        CString::new(name).expect("buffer names have no NUL")
    }
    /// `RanShaNode` for all n parties as ONE device call on the caller's own device buffers, no handle (hbmpc_dev_ransha_parties: one launch
    /// for a small batch, the handle's together form otherwise): `coeffs` [dealer][K][t + 1] or null (then `dealt` [dealer][recipient][K]
    /// is the input: `init_ransha_batch`'s received ShareMessages), `out` [party][K][n - 2t], `yv` [party][2t][K], `ws` 2 n n K +
    /// max(2t, t + 1) K elements, `bad` [2] u32 (written).  Safety: every pointer is a device buffer of the size the header states
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn ransha_parties(gpu: &GpuShares, coeffs: *const sys::U256, dealt: *mut sys::U256, batch: usize, n: usize, t: usize, out: *mut sys::U256,
                                 yv: *mut sys::U256, ws: *mut sys::U256, bad: *mut u32, stream: *mut core::ffi::c_void) -> Result<(), InterpolateError> {
        let rc = sys::hbmpc_dev_ransha_parties(gpu.ctx, coeffs, dealt, batch, n, t, 2 * t + 1, out, yv, ws, std::ptr::null_mut(), std::ptr::null_mut(), bad, stream);
        gpu.check(rc, n)
    }
    /// `DouShaNode` + `RanDouShaNode` the same way (hbmpc_dev_randousha_parties): two of every buffer, `out_*` [party][K][t + 1], `yv_*`
    /// [party][n - t - 1][K], `ws` 2 n n K + (n - t - 1) n K elements, `sel_*` 2 (n - t - 1) K elements, `st_*` (n - t - 1) K bytes
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn randousha_parties(gpu: &GpuShares, coeffs: [*const sys::U256; 2], dealt: [*mut sys::U256; 2], batch: usize, n: usize, t: usize,
                                    out: [*mut sys::U256; 2], yv: [*mut sys::U256; 2], ws: *mut sys::U256, sel: [*mut sys::U256; 2],
                                    st: [*mut core::ffi::c_void; 2], bad: *mut u32, stream: *mut core::ffi::c_void) -> Result<(), InterpolateError> {
        let rc = sys::hbmpc_dev_randousha_parties(gpu.ctx, coeffs[0], coeffs[1], dealt[0], dealt[1], batch, n, t, out[0], out[1], yv[0], yv[1], ws, sel[0], sel[1],
                                                  st[0], st[1], bad, stream);
        gpu.check(rc, n)
    }
    /// a part of a preprocessing pipeline (`"ransha"`, `"randousha"`, `"triplegen"`): borrowed, lives as long as `self`
    pub fn part(&self, name: &str) -> Result<GpuPipeline<'a>, InterpolateError> {
        let mut p = std::ptr::null_mut();
        let rc = unsafe { sys::hbmpc_pipe_part(self.pipe, Self::name(name).as_ptr(), &mut p) };
        self.gpu.check(rc, 0)?;
        Ok(GpuPipeline { gpu: self.gpu, pipe: p, owned: false })
    }
    /// device pointer and element count of a named buffer (for hosts that fill it with their own device calls)
    pub fn buffer(&self, name: &str) -> Result<(*mut sys::U256, usize), InterpolateError> {
        let (mut p, mut n) = (std::ptr::null_mut(), 0usize);
        let rc = unsafe { sys::hbmpc_pipe_buffer(self.pipe, Self::name(name).as_ptr(), &mut p, &mut n) };
        self.gpu.check(rc, 0)?;
        Ok((p as *mut sys::U256, n))
    }
    /// `[party][..]` values into a named input buffer
    pub fn upload(&self, name: &str, values: &[Fr]) -> Result<(), InterpolateError> {
        let v: Vec<sys::U256> = values.iter().map(to_u256).collect();
        let rc = unsafe { sys::hbmpc_pipe_upload(self.pipe, Self::name(name).as_ptr(), v.as_ptr() as *const core::ffi::c_void, v.len()) };
        self.gpu.check(rc, 0)
    }
    /// the first `elements` values of a named buffer (synchronises)
    pub fn download(&self, name: &str, elements: usize) -> Result<Vec<Fr>, InterpolateError> {
        let mut v = vec![sys::U256::default(); elements];
        let rc = unsafe { sys::hbmpc_pipe_download(self.pipe, Self::name(name).as_ptr(), v.as_mut_ptr() as *mut core::ffi::c_void, elements) };
        self.gpu.check(rc, 0)?;
        Ok(v.iter().map(from_u256).collect())
    }
    /// the PRandBit / PRandInt handles' buffers have element types of their own: `u64` values (contrib, b_q, sums, r_q, rb, opened) ...
    pub fn upload_u64(&self, name: &str, values: &[u64]) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_upload(self.pipe, Self::name(name).as_ptr(), values.as_ptr() as *const core::ffi::c_void, values.len()) };
        self.gpu.check(rc, 0)?;
        let rc = unsafe { sys::hbmpc_pipe_sync(self.pipe) };  // the copy reads `values`
        self.gpu.check(rc, 0)
    }
    pub fn download_u64(&self, name: &str, elements: usize) -> Result<Vec<u64>, InterpolateError> {
        let mut v = vec![0u64; elements];
        let rc = unsafe { sys::hbmpc_pipe_download(self.pipe, Self::name(name).as_ptr(), v.as_mut_ptr() as *mut core::ffi::c_void, elements) };
        self.gpu.check(rc, 0)?;
        Ok(v)
    }
    /// ... and bytes (bad, r_2, b_2, rstatus)
    pub fn download_bytes(&self, name: &str, elements: usize) -> Result<Vec<u8>, InterpolateError> {
        let mut v = vec![0u8; elements];
        let rc = unsafe { sys::hbmpc_pipe_download(self.pipe, Self::name(name).as_ptr(), v.as_mut_ptr() as *mut core::ffi::c_void, elements) };
        self.gpu.check(rc, 0)?;
        Ok(v)
    }
    /// the seeded handles' `seeds`: n seeds of 32 bytes, one per sender
    pub fn upload_bytes(&self, name: &str, bytes: &[u8]) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_upload(self.pipe, Self::name(name).as_ptr(), bytes.as_ptr() as *const core::ffi::c_void, bytes.len()) };
        self.gpu.check(rc, 0)?;
        let rc = unsafe { sys::hbmpc_pipe_sync(self.pipe) };  // the copy reads `bytes`
        self.gpu.check(rc, 0)
    }
    /// enqueue the whole pipeline on its stream
    pub fn run(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_set_checked(self.pipe, 0) };
        self.gpu.check(rc, 0)?;
        let rc = unsafe { sys::hbmpc_pipe_run(self.pipe) };
        self.gpu.check(rc, 0)
    }
    /// run and read every decode's summary back: a chunk that fails ends the run with its error, as the reference's `?` does
    pub fn run_checked(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_set_checked(self.pipe, 1) };
        self.gpu.check(rc, 0)?;
        let rc = unsafe { sys::hbmpc_pipe_run(self.pipe) };
        self.gpu.check(rc, 0)
    }
    /// checked run of a RandBit pipeline (`pipe_randbit`): phase 2's errors come back as the reference's variants
    /// (rand_bit.rs:198-207); a failed open is `Abort`, as a failed BatchRecon ends the reference's session
    pub fn randbit(&self) -> Result<(), RandBitError> {
        let rc = unsafe { sys::hbmpc_pipe_set_checked(self.pipe, 1) };
        if rc != sys::ShareSuccess {
            return Err(RandBitError::Abort);
        }
        let rc = unsafe { sys::hbmpc_pipe_run(self.pipe) };
        match rc {
            sys::ShareSuccess => Ok(()),
            sys::HBMPC_ZERO_SQUARE => Err(RandBitError::ZeroSquare),
            sys::HBMPC_NO_SQUARE_ROOT => Err(RandBitError::SquareRoot),
            _ => Err(RandBitError::Abort),
        }
    }
    /// a FixedPrep pipeline (`pipe_fixedprep`): `pairs` multiplications' worth from the front of its pools into a consumer's buffers --
    /// `rbits` [n][m][pairs] and `rint` [n][pairs] of an fpmul or truncpr pipeline (`buffer`), either may be null.  A pool that is short
    /// is `InsufficientShares`, as the reference's take_* : nothing is written and the cursors stay.
    /// Safety: the destinations are device buffers of those sizes
    pub unsafe fn take(&self, m: usize, pairs: usize, rbits: *mut sys::U256, rint: *mut sys::U256) -> Result<(), InterpolateError> {
        let rc = sys::hbmpc_pipe_fixedprep_take(self.pipe, m, pairs, rbits as *mut core::ffi::c_void, rint as *mut core::ffi::c_void);
        self.gpu.check(rc, 0)
    }
    /// a seeded pipeline: the stream position of the next `run`, which then advances it by its batch
    pub fn set_stream_index(&self, index: u64) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_set_stream_index(self.pipe, index) };
        self.gpu.check(rc, 0)
    }
    /// (bits, integers) left in a FixedPrep pipeline's pools
    pub fn available(&self) -> Result<(usize, usize), InterpolateError> {
        let mut left = [0usize; 2];
        let rc = unsafe { sys::hbmpc_pipe_fixedprep_available(self.pipe, left.as_mut_ptr()) };
        self.gpu.check(rc, 0)?;
        Ok((left[0], left[1]))
    }
    /// the two halves of a producer's run: the dealers' `compute_shares`, then everything after their messages have arrived
    pub fn deal(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_deal(self.pipe) };
        self.gpu.check(rc, 0)
    }
    pub fn finish(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_finish(self.pipe) };
        self.gpu.check(rc, 0)
    }
    /// record the call sequence as a HIP graph (after two eager runs); `replay` launches the recording
    pub fn capture(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_capture(self.pipe) };
        self.gpu.check(rc, 0)
    }
    pub fn replay(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_replay(self.pipe) };
        self.gpu.check(rc, 0)
    }
    pub fn sync(&self) -> Result<(), InterpolateError> {
        let rc = unsafe { sys::hbmpc_pipe_sync(self.pipe) };
        self.gpu.check(rc, 0)
    }
    /// the last decode's summary (synchronises)
    pub fn summary(&self) -> Result<sys::RecoverSummary, InterpolateError> {
        let mut s = sys::RecoverSummary::default();
        let rc = unsafe { sys::hbmpc_pipe_summary(self.pipe, &mut s) };
        self.gpu.check(rc, 0)?;
        Ok(s)
    }
    /// a producer's verdict: (verifier checks that failed, first failing batch element); (0, _) = every verifier says OK
    /// -- the `Ok` / abort decision of share_gen.rs:516-530 and ran_dou_sha/mod.rs:586-602 for the whole batch
    pub fn verdict(&self) -> Result<(u32, u32), InterpolateError> {
        let mut v = [0u32; 2];
        let rc = unsafe { sys::hbmpc_pipe_verdict(self.pipe, v.as_mut_ptr()) };
        self.gpu.check(rc, 0)?;
        Ok((v[0], v[1]))
    }
}

/// the process-wide context the trait impl below uses (device from HBMPC_DEVICE, default 0)
pub fn global() -> &'static Mutex<GpuShares> {
    static G: OnceLock<Mutex<GpuShares>> = OnceLock::new();
    G.get_or_init(|| {
        let dev = std::env::var("HBMPC_DEVICE").ok().and_then(|v| v.parse().ok()).unwrap_or(0);
        Mutex::new(GpuShares::new(dev).expect("libhbmpc_hip: no device"))
    })
}

/// `RobustShare<Fr>` whose scheme functions run on the GPU.  Everything else -- the share record, the operators with
/// their `IdMismatch` / `DegreeMismatch` checks (common/mod.rs:167-300) -- is the reference's own code on the inner
/// share, so `HoneyBadgerMPCNode<Fr, R>` and the sub-protocol nodes compile unchanged with this type in place of
/// `RobustShare<Fr>`.
#[derive(Clone, Debug, PartialEq)]
pub struct GpuRobustShare(pub RobustShare<Fr>);

impl From<RobustShare<Fr>> for GpuRobustShare {
    fn from(s: RobustShare<Fr>) -> Self {
        GpuRobustShare(s)
    }
}
impl Add for GpuRobustShare {
    type Output = Result<Self, ShareError>;
    fn add(self, rhs: Self) -> Self::Output {
        (self.0 + rhs.0).map(GpuRobustShare)
    }
}
impl Sub for GpuRobustShare {
    type Output = Result<Self, ShareError>;
    fn sub(self, rhs: Self) -> Self::Output {
        (self.0 - rhs.0).map(GpuRobustShare)
    }
}
impl Add<Fr> for GpuRobustShare {
    type Output = Result<Self, ShareError>;
    fn add(self, rhs: Fr) -> Self::Output {
        (self.0 + rhs).map(GpuRobustShare)
    }
}
impl Sub<Fr> for GpuRobustShare {
    type Output = Result<Self, ShareError>;
    fn sub(self, rhs: Fr) -> Self::Output {
        (self.0 - rhs).map(GpuRobustShare)
    }
}
impl Mul<Fr> for GpuRobustShare {
    type Output = Result<Self, ShareError>;
    fn mul(self, rhs: Fr) -> Self::Output {
        (self.0 * rhs).map(GpuRobustShare)
    }
}

impl SecretSharingScheme<Fr> for GpuRobustShare {
    type SecretType = Fr;
    type Error = InterpolateError;

    /// one secret = a batch of one (`ids` is ignored, as in the reference: robust_interpolate.rs:56)
    fn compute_shares(secret: Fr, n: usize, degree: usize, _ids: Option<&[usize]>, rng: &mut impl Rng)
        -> Result<Vec<Self>, InterpolateError> {
        let gpu = global().lock().expect("hbmpc context poisoned");
        let by_party = gpu.compute_shares_batch(&[secret], n, degree, rng)?;
        Ok(by_party.into_iter().map(|mut row| GpuRobustShare(row.remove(0))).collect())
    }

    fn recover_secret(shares: &[Self], n: usize, t: usize) -> Result<(Vec<Fr>, Fr), InterpolateError> {
        let inner: Vec<RobustShare<Fr>> = shares.iter().map(|s| s.0.clone()).collect();
        global().lock().expect("hbmpc context poisoned").recover_secret(&inner, n, t)
    }
}

/// `Shamirshare<Fr>` (common/share/shamir.rs:13-126: shares at the field elements `Fr::from(id as u64)`, recovery by plain
/// Lagrange) whose scheme functions run on the GPU.  The share record is the reference's own.
#[derive(Clone, Debug)]
pub struct GpuShamirshare(pub crate::common::share::shamir::Shamirshare<Fr>);

/// `ShareErrorCode` -> `ShareError`, the error type of `Shamirshare` (shamir.rs:42)
fn share_error(rc: sys::ShareErrorCode) -> Result<(), ShareError> {
    match rc {
        sys::ShareSuccess => Ok(()),
        sys::InsufficientShares => Err(ShareError::InsufficientShares),
        sys::DegreeMismatch => Err(ShareError::DegreeMismatch),
        sys::IdMismatch => Err(ShareError::IdMismatch),
        sys::TypeMismatch => Err(ShareError::TypeMismatch),
        _ => Err(ShareError::InvalidInput), // InvalidInput and the library's own codes (no device, out of memory)
    }
}

impl GpuShares {
    /// `B` calls of `Shamirshare::compute_shares` (shamir.rs:44-88) in one launch, the rng drawn as the reference draws it per
    /// secret.  Returns `[id i][secret b]`.  The checks, in the reference's order, are the library's (include/hbmpc_hip.h).
    pub fn shamir_compute_shares_batch(&self, secrets: &[Fr], degree: usize, ids: Option<&[usize]>, rng: &mut impl Rng)
        -> Result<Vec<Vec<crate::common::share::shamir::Shamirshare<Fr>>>, ShareError> {
        use crate::common::share::shamir::Shamirshare;
        let b = secrets.len();
        let points: Option<Vec<u64>> = ids.map(|l| l.iter().map(|&i| i as u64).collect());
        let (pp, m) = points.as_ref().map_or((std::ptr::null(), 0), |p| (p.as_ptr(), p.len()));
        // the id checks come before DensePolynomial::rand in the reference: a refused call consumes no draw (B = 0 checks only)
        share_error(unsafe { sys::hbmpc_shamir_compute_shares(self.ctx, std::ptr::null(), 0, pp, m, degree, std::ptr::null_mut()) })?;
        let mut coeffs = Vec::<sys::U256>::with_capacity(b * (degree + 1));
        for s in secrets {
            let mut poly = DensePolynomial::<Fr>::rand(degree, rng); // (:73)
            poly.coeffs[0] = *s; // (:74)
            coeffs.extend(poly.coeffs.iter().map(to_u256));
        }
        let mut out = vec![sys::U256::default(); m * b];
        share_error(unsafe { sys::hbmpc_shamir_compute_shares(self.ctx, coeffs.as_ptr(), b, pp, m, degree, out.as_mut_ptr()) })?;
        let ids = ids.unwrap_or(&[]);
        Ok((0..m)
            .map(|i| out[i * b..(i + 1) * b].iter().map(|v| Shamirshare::new(from_u256(v), ids[i], degree)).collect())
            .collect())
    }

    /// `Shamirshare::recover_secret` (shamir.rs:90-125), the checks in its order
    pub fn shamir_recover_secret(&self, shares: &[crate::common::share::shamir::Shamirshare<Fr>]) -> Result<(Vec<Fr>, Fr), ShareError> {
        let s = shares.len();
        let ids: Vec<u64> = shares.iter().map(|x| x.id as u64).collect();
        let degrees: Vec<usize> = shares.iter().map(|x| x.degree).collect();
        let vals: Vec<sys::U256> = shares.iter().map(|x| to_u256(&x.share[0])).collect();
        let mut coeffs = vec![sys::U256::default(); s.max(1)];
        let mut ncoeffs: usize = 0;
        let mut secret = sys::U256::default();
        share_error(unsafe {
            sys::hbmpc_shamir_recover_secret(self.ctx, ids.as_ptr(), degrees.as_ptr(), vals.as_ptr(), s, coeffs.as_mut_ptr(), &mut ncoeffs,
                                             &mut secret)
        })?;
        Ok((coeffs[..ncoeffs].iter().map(from_u256).collect(), from_u256(&secret)))
    }
}

impl SecretSharingScheme<Fr> for GpuShamirshare {
    type SecretType = Fr;
    type Error = ShareError;

    /// one secret = a batch of one; `_n` is unused, as in the reference (shamir.rs:46)
    fn compute_shares(secret: Fr, _n: usize, degree: usize, ids: Option<&[usize]>, rng: &mut impl Rng) -> Result<Vec<Self>, ShareError> {
        let gpu = global().lock().expect("hbmpc context poisoned");
        let by_id = gpu.shamir_compute_shares_batch(&[secret], degree, ids, rng)?;
        Ok(by_id.into_iter().map(|mut row| GpuShamirshare(row.remove(0))).collect())
    }

    fn recover_secret(shares: &[Self], _n: usize, _t: usize) -> Result<(Vec<Fr>, Fr), ShareError> {
        let inner: Vec<_> = shares.iter().map(|s| s.0.clone()).collect();
        global().lock().expect("hbmpc context poisoned").shamir_recover_secret(&inner)
    }
}
