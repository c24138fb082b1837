/* part of sf3d_solver.hip (included there, in this order: physics, control, phases, host_build, host_step) - the node kernels of a water step: k_props, k_assemble, k_sweep (+ the paired sweeps), k_post, k_restore, k_accept*, k_storage */
/* ======================================================================================= */
/* node kernels: one wave64 walks 64-node chunks (grid-stride), one lane per node            */
/* ======================================================================================= */

/* chunk loop: q is wave-uniform (forced into an SGPR so descriptor loads go through the scalar path) */
#define FOR_EACH_CHUNK_OF(list, l0, l1)                                                           \
    const uint32_t lane_ = threadIdx.x & 63u;                                                     \
    const uint32_t wavesTotal_ = gridDim.x * (SF3D_BLOCK / 64);                                   \
    for (uint32_t li_ = __builtin_amdgcn_readfirstlane((l0) + blockIdx.x * (SF3D_BLOCK / 64) + (threadIdx.x >> 6)); \
         li_ < (l1); li_ += wavesTotal_)                                                          \
        for (uint32_t q = __builtin_amdgcn_readfirstlane((list)[li_]), once_ = 1; once_; once_ = 0)
#define FOR_EACH_CHUNK_IN(v, l0, l1) FOR_EACH_CHUNK_OF((v).chunkList, l0, l1)
/* chunks this rank owns (all of them on one GPU), their surface part, their soil part */
#define FOR_EACH_CHUNK(v) FOR_EACH_CHUNK_IN(v, 0u, (v).nList)
/* lane-level ownership: strips are cut at chunk boundaries whenever the numbering allows it, the
 * per-node owner map covers the general case */
#define NOT_MINE(v, i) ((i) >= (v).N || ((v).owner != nullptr && (v).owner[i] != (v).rank))

#include "sf3d_heat.inc"

/* ---- waterFlow = sink (+ evaporation clamp) + boundary flow (water.cpp:632-807) ---- */
template <bool HEAT>
__device__ __forceinline__ double boundary_update(const DevView& v, const Ctrl* c, uint32_t i, double H, double Ho,
                                                  double z, double K, double Se)
{
    const double dt = c->dt;
    double flow = v.sink[i];
    if (i < v.ns && flow < 0) {                                       /* :646-652 */
        const double avgH = 0.5 * (H + Ho);
        const double hs = dmax(0., avgH - z);
        const double maxFlux = -hs * v.size[i] / dt;
        flow = dmax(flow, maxFlux);
    }
    const uint8_t bt = v.btype[i];
    double rate = 0.;
    if (bt != SF3D_BND_NONE) {
        switch (bt) {
            case SF3D_BND_RUNOFF: {                                   /* :661-678 */
                const double avgH = 0.5 * (H + Ho);
                const double hs = dmax(0., avgH - (z + v.pond[i]));
                if (hs < 0.001) break;
                const double maxFlow = (hs * v.size[i]) / dt;
                const double vel = ppow(hs, 2. / 3.) * sqrt(v.bslope[i]) / v.roughness[v.cls[i]];
                const double val = hs * vel * v.bsize[i];
                rate = -dmin(val, maxFlow);
                break; }
            case SF3D_BND_FREE_DRAINAGE:                              /* :680-684, Up-link area */
                rate = -K * v.larea[i];
                break;
            case SF3D_BND_FREE_LATERAL_DRAINAGE:                      /* :686-690 */
                rate = -K * v.bsize[i] * v.bslope[i] * c->lvRatio;
                break;
            case SF3D_BND_PRESCRIBED_TOTAL_POTENTIAL: {               /* :692-706 */
                const SoilDev s = v.soils[v.cls[i]];
                const double L = 1.;
                const double bz = z - L;
                const double pH = v.prescribed[i];
                const double bpsi = pH - bz;
                const double bK = (bpsi >= 0) ? s.Ksat : mualem_k(s, se_from_psi(s, fabs(bpsi), c->wrc), c->wrc);
                const double mk = mean_of(bK, K, c->meanType);
                rate = mk * v.bsize[i] * ((pH - H) / L);
                break; }
            case SF3D_BND_HEAT_SURFACE: {                             /* :708-747: soil evaporation / condensation */
                if (!HEAT || !v.heat.vapor) break;
                const HeatDev& hv = v.heat;
                const SoilDev s = v.soils[v.cls[i]];
                const uint32_t up = v.lto[i];                         /* slot 0; node 0 when there is no Up link, like the reference */
                const bool upLinked = v.lkind[i] != LK_NONE;
                double frac = 0.;
                if (upLinked && up < v.ns) {                          /* getNodeSurfaceWaterFraction, soilPhysics.cpp:317-326 */
                    const double hV = dmax(0., v.X[c->cur][up] - v.z[up]);
                    frac = dmin(1., hV / dmax(0.001, v.pond[up]));
                }
                double evap = 0.;
                if (up < v.ns) {                                      /* computeNodeAtmosphericLatentVaporFlux, heat.cpp:988-1008 */
                    const double Ta = hv.bT[i];
                    const double satC = h_vapor_conc_from_pressure(h_sat_vapor_pressure(Ta - H_ZEROC), Ta);
                    const double boundaryVapor = satC * (hv.bRH[i] / 100.);
                    const double dVapor = boundaryVapor - h_vapor_from_psi_temp(H - z, hv.TX[c->tCur][i]);
                    const double total = 1. / ((1. / hv.bAero[i]) + (1. / hv.bSoilCond[i]));
                    evap = dVapor * total;
                }
                evap = evap / H_RHOW * v.larea[i];
                if (frac > 0.) evap *= (1. - frac);
                const double thetaV = (Se * (s.thetaS - s.thetaR)) + s.thetaR;
                rate = (evap < 0.) ? dmax(evap, -(thetaV - s.thetaR) * v.size[i] / dt)
                                   : dmin(evap, (s.thetaS - s.thetaR) * v.size[i] / dt);
                break; }
            default: rate = 0.; break;                                /* Urban/Road/Culvert */
        }
        if (fabs(rate) < DBL_EPSILON) rate = 0.;                      /* :802-805 */
        else flow += rate;
    }
    if (HEAT && i < v.ns && v.heat.vapor && v.lkind[(size_t)v.N + i] != LK_NONE) {
        /* evaporation of ponded water (water.cpp:719-733).  The reference lets the HeatSurface node below write
         * into this node; here the surface node pulls: same values, same order (this node's own boundary first) */
        const HeatDev& hv = v.heat;
        const uint32_t d = v.lto[(size_t)v.N + i];                    /* slot 1 = Down */
        if (v.btype[d] == SF3D_BND_HEAT_SURFACE && v.lkind[d] != LK_NONE && v.lto[d] == i) {
            const double hV = dmax(0., H - z);
            const double frac = dmin(1., hV / dmax(0.001, v.pond[i]));
            if (frac > 0.) {                                          /* computeNodeAtmosphericLatentSurfaceWaterFlux, heat.cpp:1014-1039 */
                const double Ta = hv.bT[d];
                const double satC = h_vapor_conc_from_pressure(h_sat_vapor_pressure(Ta - H_ZEROC), Ta);
                const double boundaryVapor = satC * (hv.bRH[d] / 100.);
                double surfEvap = ((boundaryVapor - satC) * hv.bAero[d]) / H_RHOW * v.larea[d];
                surfEvap *= frac;
                const double volume = (H - z) * v.size[i];
                surfEvap = dmax(surfEvap, -volume / dt);
                if (bt != SF3D_BND_NONE) rate = surfEvap;             /* overwrites the rate, waterFlow keeps the runoff already added */
                else flow += surfEvap;
            }
        }
    }
    if (bt != SF3D_BND_NONE) v.bflowRate[i] = rate;
    v.flow[i] = flow;
    return flow;
}


/* dtheta/dH with the two saturation degrees already known (soilPhysics.cpp:224-279):
 * Se(psiCurr) is the Se array (post-solve of the previous approximation, same H) and Se(psiPrev)
 * is SeHold (written at approximation 0, when H == Hold) - the same values the reference
 * recomputes with four pow calls per node per approximation. */
__device__ __forceinline__ double dtheta_dh_cached(const SoilDev& s, double H, double Ho, double z, uint32_t wrc,
                                                   double SeCur, double SePrev)
{
    const double psiCurr = fabs(dmin(0.0, H - z));
    const double psiPrev = fabs(dmin(0.0, Ho - z));
    if (wrc == SF3D_WRC_VAN_GENUCHTEN) { if (psiCurr == 0.0 && psiPrev == 0.0) return 0.0; }
    else if (wrc == SF3D_WRC_MODIFIED_VAN_GENUCHTEN) { if (psiCurr <= s.he && psiPrev <= s.he) return 0.0; }
    double dSe;
    if (fabs(psiCurr - psiPrev) < 1e-12) {
        const double xx = s.alpha * psiCurr;
        const double onePlus = 1. + ppow(xx, s.n);
        const double t1 = ppow(onePlus, -(s.m + 1.));
        const double t2 = ppow(xx, s.n - 1.);
        dSe = s.alpha * s.n * s.m * t1 * t2;
        if (wrc == SF3D_WRC_MODIFIED_VAN_GENUCHTEN) dSe *= s.invSc;
    } else
        dSe = fabs((SeCur - SePrev) / (H - Ho));
    return dSe * (s.thetaS - s.thetaR);
}

/* computeCapacity (water.cpp:279-297) + step-begin Se (cpusolver.cpp:165-169) +
 * updateBoundaryWaterData (water.cpp:632-807) */
#ifndef SF3D_PROPS_HEAT_WAVES
#define SF3D_PROPS_HEAT_WAVES 4     /* 128 VGPRs, no scratch (left to itself the compiler takes 131 with the library-faithful pow: three waves) */
#endif
#ifndef SF3D_PROPS_WAVES
#define SF3D_PROPS_WAVES 5     /* 96 VGPRs, no scratch on one GPU (the table-driven pow needs fewer registers than the library's):
                                * 150 -> 135 us at C4 against 4 waves, launched with exactly the 1 280 resident blocks */
#endif
template <int MODE, bool HEAT>
__device__ __forceinline__ void body_props(const DevView& v)
{
    const Ctrl* c = v.ctrl;
    fm_init();
    const double* __restrict__ Xc = v.X[c->cur];
    const double* __restrict__ Xh = v.X[c->hold];
    const uint32_t wrc = c->wrc;
    const uint32_t par = c->epoch & 1u;
    const bool first = c->approx == 0;
    const uint32_t seSource = c->seSource;
    FOR_EACH_CHUNK_IN(v, v.pLo, v.pHi) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        const bool mine = !NOT_MINE(v, i);
        double K = 0., fl = 0.;
        if (mine) {
            const double H = Xc[i], Ho = Xh[i], z = v.z[i];
            double Se = 1.;
            if (i >= v.ns) {
                const SoilDev s = v.soils[v.cls[i]];
                double SeH;
                if (first) {
                    /* cpusolver.cpp:165-169 recomputes Se(H) at the head of every attempt; the same function of the same H was
                     * already evaluated by k_post / k_restore (accepted step) or by the refused attempt: reuse those bits */
                    Se = (seSource == 1) ? v.Se[i] : (seSource == 2) ? v.SeHold[i] : node_se(s, H, z, wrc);
                    SeH = Se; v.Se[i] = Se; v.SeHold[i] = Se;
                }
                else { Se = v.Se[i]; SeH = v.SeHold[i]; }
                K = mualem_k(s, Se, wrc);
                const double dThdH = dtheta_dh_cached(s, H, Ho, z, wrc, Se, SeH);
                double C = v.size[i] * dThdH;
                if (HEAT) {                                   /* vapour terms of computeNodeK / computeCapacity + the node
                                                                 conductivities of the thermal fluxes in the water rows */
                    const HeatDev& hv = v.heat;
                    const double Tm = (hv.TX[c->tCur][i] + hv.TX[c->tOld][i]) * 0.5;   /* getNodeMeanTemperature */
                    const double h = H - z;
                    const double theta = h_theta_signed_psi(s, h, wrc);
                    if (hv.vapor) {
                        K += h_isothermal_vapor_conductivity(s, Tm, h, theta) * (H_G / H_RHOW);
                        C += v.size[i] * h_dthetav_dh(s, h, Tm, dThdH, wrc);
                        hv.wThVap[i] = h_thermal_vapor_conductivity(s, hv.airP[i], Tm, h, theta);
                    }
                    hv.wTm[i] = Tm;
                    hv.wThLiq[i] = h_thermal_liquid_conductivity(Tm - H_ZEROC, h, K);
                }
                v.K[i] = K;
                v.C[i] = C;
            }
            boundary_update<HEAT>(v, c, i, H, Ho, z, K, Se);
            if (MODE == 2) fl = v.flow[i];
        }
        /* multi GPU: K and waterFlow of the boundary nodes go to the neighbours as tagged records - k_halo_copy<0> (next launch, many blocks)
         * waits for the tags and copies them in before the assembly reads neighbours; no barrier across the ranks, no exchange epoch
         * (rounds 3-5: plain puts, a mailbox round of the last block, then the copy: 133 of an episode's 1 103 epochs) */
        if (MODE == 2) dist_put_chunk_kf(v, q, lane_, par, c->epoch + 1u, K, fl);
    }
}
template <int MODE, bool HEAT>
__global__ void __launch_bounds__(SF3D_BLOCK, HEAT ? SF3D_PROPS_HEAT_WAVES : SF3D_PROPS_WAVES) k_props(DevView v)
{
    if (v.ctrl->stage != ST_APPROX) return;
    body_props<MODE, HEAT>(v);
}

/* The halo copies that used to run in the ONE block that closes an exchange (20 000 system-scope loads at 8-way C4,
 * tens of microseconds on the critical path of every approximation) as a launch of their own with many blocks.
 * WHAT 0: K and waterFlow after k_props; WHAT 1: the final iterate of the sweeps after k_post.  Each copy is tied to the
 * epoch its exchange closed, so a launch queued in vain (guarded no-op batches) copies nothing stale. */
template <int WHAT>
__global__ void __launch_bounds__(SF3D_BLOCK) k_halo_copy(DevView v)
{
    const Ctrl* c = v.ctrl;
    if (v.world <= 1) return;
    const DistView* d = v.dist;
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    if (WHAT == 0) {
        /* K and waterFlow arrive as tagged records (k_props<2>, tag = the epoch both launches run in + 1): every thread waits for its own -
         * bounded; a record that does not come is a failed step (the peer's next mailbox round runs into its bound as well) */
        if (c->stage != ST_APPROX) return;
        const uint32_t par = c->epoch & 1u, tag = c->epoch + 1u;
        for (int p = 0; p < v.world; ++p) {
            const uint32_t cnt = d->recvCount[p];
            const uint32_t* idx = d->recvIdx[p];
            const double* base = d->payload[v.rank] + d->recvOff[p] + (size_t)(par * SF3D_DIST_FIELDS) * cnt;
            for (uint32_t k = tid; k < cnt; k += nth) {
                const uint32_t i = idx[k];
                const double *k0 = &base[(size_t)DF_KLO * cnt + k], *k1 = &base[(size_t)DF_KHI * cnt + k], *f0 = &base[(size_t)DF_FLO * cnt + k], *f1 = &base[(size_t)DF_FHI * cnt + k];
                long long t0 = 0;
                for (uint32_t polls = 0;; ++polls) {
                    const unsigned long long a = (unsigned long long)__double_as_longlong(SYS_LOAD(k0)), b = (unsigned long long)__double_as_longlong(SYS_LOAD(k1));
                    const unsigned long long e = (unsigned long long)__double_as_longlong(SYS_LOAD(f0)), f = (unsigned long long)__double_as_longlong(SYS_LOAD(f1));
                    if (rec_ok(a, b, tag) && rec_ok(e, f, tag)) { v.K[i] = rec_value(a, b); v.flow[i] = rec_value(e, f); break; }
                    if (polls == 0) t0 = wall_clock64();
                    __builtin_amdgcn_s_sleep(2);
                    if ((polls & 63u) == 63u && (wall_clock64() - t0 > d->spinTicks || __hip_atomic_load(&v.ctrl->distError, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                        Ctrl* w = v.ctrl;
                        atomicOr(&w->distError, 1u); atomicOr(&w->distSilent, 1u << p); w->stage = ST_FAIL;
                        return;
                    }
                }
            }
        }
    } else {
        if (c->haloEpoch != c->epoch) return;
        double* __restrict__ dst = v.X[c->haloBuf];
        const uint32_t par = c->haloPar;
        for (int p = 0; p < v.world; ++p) {
            const uint32_t cnt = d->recvCount[p];
            const uint32_t* idx = d->recvIdx[p];
            const double* src = d->payload[v.rank] + d->recvOff[p] + (size_t)(par * SF3D_DIST_FIELDS + DF_X) * cnt;
            for (uint32_t k = tid; k < cnt; k += nth) dst[idx[k]] = SYS_LOAD(&src[k]);
        }
    }
}

/* infiltration, water.cpp:490-539: one end is a surface node, the other a soil node */
__device__ __forceinline__ double infiltration_conductance(const DevView& v, const Ctrl* c, uint32_t i, uint32_t j, size_t e,
                                                           const double* __restrict__ Xc, const double* __restrict__ Xh,
                                                           double Hi, double Hoi, double zi)
{
    const double area = v.larea[e], dist = v.ldist[e];
    const double dt = c->dt;
    const bool iSurf = i < v.ns;
    const uint32_t su = iSurf ? i : j, so = iSurf ? j : i;
    const double Hsu = iSurf ? Hi : Xc[j], Hosu = iSurf ? Hoi : Xh[j];
    const double Hso = iSurf ? Xc[j] : Hi, Hoso = iSurf ? Xh[j] : Hoi;
    const double zsu = iSurf ? zi : v.z[j];
    const SoilDev s = v.soils[v.cls[so]];
    double factor = 1.;
    const uint8_t bt = v.btype[so];
    if (bt == SF3D_BND_URBAN) factor = 0.33;
    else if (bt == SF3D_BND_ROAD) return 0.;
    if (Hso > zsu) return (s.Ksat * factor * area) / dist;
    const double surfH = 0.5 * (Hsu + Hosu);
    const double soilH = 0.5 * (Hso + Hoso);
    double surfaceWater = dmax(surfH - zsu, 0.);
    const double qf = v.flow[su];
    if (qf < 0.) {
        const double bm = (qf * dt) / v.size[su];
        surfaceWater = dmax(0., surfaceWater + bm);
    }
    const double maxInfRate = surfaceWater / dt;
    if (maxInfRate < 2.78e-11) return 0.;
    const double dH = dmax(surfH - soilH, 1e-12);
    const double maxK = maxInfRate * (dist / dH);
    const double meanK = mean_of(s.Ksat, v.K[so], c->meanType);
    return (dmin(factor * meanK, maxK) * area) / dist;
}

/* link conductances: water.cpp:300-343 dispatch, :413-487 runoff, :490-539 infiltration,
 * :542-562 redistribution */
__device__ __forceinline__ double link_conductance(const DevView& v, const Ctrl* c, uint32_t i, uint32_t j, size_t e,
                                                   uint8_t kind, const double* __restrict__ Xc,
                                                   const double* __restrict__ Xh, double Hi, double Hoi,
                                                   double zi, double& courant)
{
    const double area = v.larea[e], dist = v.ldist[e];
    const double dt = c->dt;
    if (kind == LK_SOIL_VERT || kind == LK_SOIL_LAT) {
        double ki = v.K[i], kj = v.K[j];
        if (kind == LK_SOIL_LAT) { ki *= c->lvRatio; kj *= c->lvRatio; }
        return qdiv(mean_of(ki, kj, c->meanType) * area, dist);
    }
    if (kind == LK_RUNOFF) {
        double Ha = 0.5 * (Hi + Hoi);
        double Hb = 0.5 * (Xc[j] + Xh[j]);
        if (c->approx == 0) {
            const double fi = v.flow[i], fj = v.flow[j];
            if (fi > 0) Ha += 0.5 * fi * dt / v.size[i];
            if (fj > 0) Hb += 0.5 * fj * dt / v.size[j];
        }
        const double za = zi + v.pond[i], zb = v.z[j] + v.pond[j];
        const double Hs = dmax(Ha, Hb) - dmax(za, zb);
        if (Hs <= 0.00001) return 0.0;
        if (dist <= 0.0) return 0.0;
        const double rough = 0.5 * (v.roughness[v.cls[i]] + v.roughness[v.cls[j]]);
        if (rough <= 0.0) return 0.0;
        const double Aw = area * Hs;
        const double Hs23 = pcbrt(Hs * Hs);
        const double Kij = Aw * Hs23 / (rough * dist);
        const double dH = fabs(Ha - Hb);
        const double slope = (dH > 0.00001) ? dH / dist : 0.0;
        const double vel = Hs23 * sqrt(slope) / rough;
        courant = dmax(courant, vel * dt / dist);
        return Kij;
    }
    return infiltration_conductance(v, c, i, j, e, Xc, Xh, Hi, Hoi, zi);
}

/* computeLinearSystemElement (cpusolver.cpp:348-389, order Up, laterals, Down) +
 * computeDiagonalElement (:335-345) + preconditioningMatrix (:284-305), in two kernels like the
 * reference's two loops (surface rows, Courant check, soil rows - cpusolver.cpp:412-429). */
/* thermal liquid (+ vapour) flux of one soil-soil link in the water rows: computeThermalLiquidFlux /
 * computeThermalVaporFlux with processType::Water (heat.cpp:469-567), added to invariantFluxes (water.cpp:328-340) */
__device__ __forceinline__ void add_thermal_fluxes(const HeatDev& hv, uint32_t i, uint32_t j, double area, double dist3, double& inv)
{
    const double Ti = hv.wTm[i], Tj = hv.wTm[j];
    const double avgL = mean_of(hv.wThLiq[i], hv.wThLiq[j], SF3D_MEAN_LOGARITHMIC);
    inv += (avgL * (Tj - Ti) / dist3) * area;
    if (hv.vapor) {
        const double avgV = mean_of(hv.wThVap[i], hv.wThVap[j], SF3D_MEAN_LOGARITHMIC);
        inv += ((avgV * (Tj - Ti) / dist3) * area) / H_RHOW;
    }
}

/* the same with the six node values already in registers (assemble_soil_rows<HEAT> gathers them with the link's other operands) */
__device__ __forceinline__ void add_thermal_fluxes_of(bool vapor, double Ti, double Li, double Vi, double Tj, double Lj, double Vj, double area, double dist3, double& inv)
{
    const double avgL = mean_of(Li, Lj, SF3D_MEAN_LOGARITHMIC);
    inv += (avgL * (Tj - Ti) / dist3) * area;
    if (vapor) {
        const double avgV = mean_of(Vi, Vj, SF3D_MEAN_LOGARITHMIC);
        inv += ((avgV * (Tj - Ti) / dist3) * area) / H_RHOW;
    }
}

/* scales the row (preconditioningMatrix, cpusolver.cpp:284-305), stores it, and leaves the scaled coefficients in k
 * and the right-hand side in the return value for the fused first sweep */
template <bool NT>
__device__ __forceinline__ double store_row(const DevView& v, sf3d_d2* __restrict__ A2w, const ChunkDesc& cd, uint32_t i, double (&k)[SF3D_SLOTS],
                                            double sum, double Hoi, double dt, double invariantFlux, double Ci, double flowi)
{
    const double cdt = Ci / dt;
    const bool raw = v.compatDiag != nullptr;          /* compat: row stored un-normalised, k_compat_rows scales it after the Courant decision */
    const double inv = raw ? 1.0 : 1.0 / (cdt + sum);  /* (x * 1.0 is exact) */
    if (raw) v.compatDiag[i] = cdt + sum;
    if (v.cgDiag != nullptr) v.cgDiag[i] = cdt + sum;
    #pragma unroll
    for (int p = 0; p < SF3D_SLOTS / 2; ++p) {
        k[2 * p] = (k[2 * p] * -1.) * inv; k[2 * p + 1] = (k[2 * p + 1] * -1.) * inv;
        if (cd.kind[2 * p] != CK_NONE || cd.kind[2 * p + 1] != CK_NONE) store_coeff<NT>(&A2w[(size_t)p * v.N + i], k[2 * p], k[2 * p + 1]);
    }
    const double bi = ((cdt * Hoi) + flowi + invariantFlux) * inv;   /* invariantFluxes: 0 without heat (cpusolver.cpp:148,387) */
    v.b[i] = bi;
    return bi;
}

/* rows of chunks [0, qSplit): every surface node (runoff + infiltration links) and, when
 * nrSurfaceNodes is not a multiple of 64, the first soil nodes; any link kind; Courant maximum */
template <bool NT, bool HEAT, bool COURANT_ONLY = false>       /* COURANT_ONLY: the runoff links' Courant maximum and nothing else (early check) */
__device__ __forceinline__ double assemble_surface_rows(const DevView& v, uint32_t blk, uint32_t nblk)
{
    const Ctrl* c = v.ctrl;
    const double* __restrict__ Xc = v.X[c->cur];
    const double* __restrict__ Xh = v.X[c->hold];
    sf3d_d2* __restrict__ A2w = cur_A2(v);
    const double dt = c->dt;
    constexpr uint32_t order[SF3D_SLOTS] = {0, 2, 3, 4, 5, 6, 7, 8, 9, 1};
    double courant = 0.;
    const uint32_t lane_ = threadIdx.x & 63u;
    for (uint32_t li_ = __builtin_amdgcn_readfirstlane(blk * (SF3D_BLOCK / 64) + (threadIdx.x >> 6)); li_ < v.nListSurf;
         li_ += nblk * (SF3D_BLOCK / 64)) {
        const uint32_t q = __builtin_amdgcn_readfirstlane(v.asmList[li_]);
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i)) continue;
        const ChunkDesc cd = v.cdesc[q];
        const double Hi = Xc[i], Hoi = Xh[i], zi = v.z[i];
        const double Ci = (i < v.ns) ? v.size[i] : v.C[i], flowi = v.flow[i];     /* surface capacity = area, cpusolver.cpp:151 */
        const uint32_t pmask = (COURANT_ONLY && i < v.ns) ? v.probeMask[i] : 0u;
        double k[SF3D_SLOTS];
        double sum = 0., invFlux = 0.;
        #pragma unroll
        for (int o = 0; o < SF3D_SLOTS; ++o) {
            const uint32_t s = order[o];
            double ks = 0.;
            if (cd.kind[s] != CK_NONE) {
                const size_t e = (size_t)s * v.N + i;
                uint8_t kind; uint32_t j;
                if (cd.kind[s] != CK_MIXED) { kind = cd.kind[s]; j = i + cd.delta[s]; }
                else if ((cd.sweepUniform >> s) & 1u) { kind = v.lkind[e]; const uint32_t jj = i + (uint32_t)cd.delta[s]; j = jj < v.N ? jj : i; }
                else { kind = v.lkind[e]; j = v.lto[e]; }
                if (COURANT_ONLY) { if (kind == LK_RUNOFF && s >= 2 && ((pmask >> (s - 2)) & 1u)) link_conductance(v, c, i, j, e, kind, Xc, Xh, Hi, Hoi, zi, courant); continue; }
                if (kind != LK_NONE) ks = link_conductance(v, c, i, j, e, kind, Xc, Xh, Hi, Hoi, zi, courant);
                if (HEAT && (kind == LK_SOIL_VERT || kind == LK_SOIL_LAT)) add_thermal_fluxes(v.heat, i, j, v.larea[e], v.heat.hdist[e], invFlux);
            }
            k[s] = ks;
            sum += ks;
        }
        if (!COURANT_ONLY) store_row<NT>(v, A2w, cd, i, k, sum, Hoi, dt, invFlux, Ci, flowi);
    }
    return block_max(courant);
}

/* rows of the soil-only chunks [qSplit, nChunks).  Two groups of five slots: all index / area /
 * distance loads and neighbour-K gathers of a group are issued before its first logarithm, so
 * ~20 loads per lane overlap instead of forming dependent round trips (4 waves/SIMD). */
#ifndef SF3D_ASM_HEAT_WAVES
#define SF3D_ASM_HEAT_WAVES 4
#endif
#ifndef SF3D_ASM_SCHED_BARRIER
#define SF3D_ASM_SCHED_BARRIER 1
#endif
#ifndef SF3D_ASM_WAVES
#define SF3D_ASM_WAVES 4
#endif
#ifndef SF3D_ASM_GROUPS
#define SF3D_ASM_GROUPS 2      /* 2 groups of 5 slots (5 groups of 2, 1 of 10: tuning experiments) */
#endif
#ifndef SF3D_ASM_HEAT_GROUPS
#define SF3D_ASM_HEAT_GROUPS 5 /* with heat: 5 groups of 2 slots */
#endif
template <bool NT, bool HEAT>
__device__ __forceinline__ void assemble_soil_rows(const DevView& v, uint32_t blk, uint32_t nblk)
{
    const Ctrl* c = v.ctrl;
    const double* __restrict__ Xc = v.X[c->cur];
    const double* __restrict__ Xh = v.X[c->hold];
    const double dt = c->dt, lvRatio = c->lvRatio;
    sf3d_d2* __restrict__ A2w = cur_A2(v);
    const uint32_t meanType = c->meanType;
    constexpr uint32_t order[SF3D_SLOTS] = {0, 2, 3, 4, 5, 6, 7, 8, 9, 1};
    const uint32_t lane_ = threadIdx.x & 63u;
    for (uint32_t li_ = __builtin_amdgcn_readfirstlane(v.aLo + blk * (SF3D_BLOCK / 64) + (threadIdx.x >> 6)); li_ < v.aHi;
         li_ += nblk * (SF3D_BLOCK / 64)) {
        const uint32_t q = __builtin_amdgcn_readfirstlane(v.asmList[li_]);
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i)) continue;
        const ChunkDesc cd = v.cdesc[q];                                    /* wave-uniform: scalar load */
        const double Hoi = Xh[i], Ki = v.K[i];
        const double Ci = v.C[i], flowi = v.flow[i];       /* for the row's diagonal and right-hand side: requested with the first loads, not after the last logarithm */
        double k[SF3D_SLOTS];
        double sum = 0., invFlux = 0.;
        /* with heat every soil-soil link adds its thermal liquid (+ vapour) flux: three more gathers, the 3-D distance and two more logarithmic
         * means per link.  They travel with the link's other operands, in groups of TWO slots (four more doubles per slot in flight) - read
         * inside the per-link arithmetic, one link after the other, the rows took 888 us per launch at the Ravone project against 354 us
         * without heat (profiles/README.md round 4) */
        constexpr int NG = HEAT ? SF3D_ASM_HEAT_GROUPS : SF3D_ASM_GROUPS;
        double wTi = 0., wLi = 0., wVi = 0.;
        if (HEAT) { wTi = v.heat.wTm[i]; wLi = v.heat.wThLiq[i]; wVi = v.heat.vapor ? v.heat.wThVap[i] : 0.; }
        #pragma unroll
        for (int g = 0; g < NG; ++g) {
            constexpr int GS = SF3D_SLOTS / NG;          /* slots per group */
            uint32_t j[GS]; uint8_t kd[GS];
            double area[GS], dist[GS], kj[GS];
            double d3[GS], wT[GS], wL[GS], wV[GS];       /* HEAT only */
            #pragma unroll
            for (int t = 0; t < GS; ++t) {
                const uint32_t s = order[g * GS + t];
                kd[t] = LK_NONE; j[t] = i; area[t] = 0.; dist[t] = 1.; d3[t] = 1.;
                if (cd.kind[s] != CK_NONE) {
                    const size_t e = (size_t)s * v.N + i;
                    if (cd.kind[s] != CK_MIXED) { kd[t] = cd.kind[s]; j[t] = i + cd.delta[s]; }
                    else if ((cd.sweepUniform >> s) & 1u) {     /* row end: one offset for the nodes that have the link - the gather does not wait for an index */
                        kd[t] = load_stream<NT>(&v.lkind[e]);
                        const uint32_t jj = i + (uint32_t)cd.delta[s];
                        j[t] = jj < v.N ? jj : i;
                    } else { kd[t] = load_stream<NT>(&v.lkind[e]); j[t] = load_stream<NT>(&v.lto[e]); }
                    area[t] = ((cd.areaUniform >> s) & 1u) ? cd.area[s] : load_stream<NT>(&v.larea[e]);
                    dist[t] = load_stream<NT>(&v.ldist[e]);
                    if (HEAT) d3[t] = load_stream<NT>(&v.heat.hdist[e]);      /* (1 where the link joins no two soil nodes) */
                }
            }
            #pragma unroll
            for (int t = 0; t < GS; ++t) {
                kj[t] = v.K[j[t]];
                if (HEAT) { wT[t] = v.heat.wTm[j[t]]; wL[t] = v.heat.wThLiq[j[t]]; wV[t] = v.heat.vapor ? v.heat.wThVap[j[t]] : 0.; }
            }
            #pragma unroll
            for (int t = 0; t < GS; ++t) {
                const uint32_t s = order[g * GS + t];
                double ks = 0.;
                const double dd = dist[t];
                if (kd[t] == LK_SOIL_LAT) {                                  /* redistribution, water.cpp:542-562 */
                    const double ki = Ki * lvRatio, kn = kj[t] * lvRatio;
                    ks = qdiv(mean_of(ki, kn, meanType) * area[t], dd);
                } else if (kd[t] == LK_SOIL_VERT) {
                    ks = qdiv(mean_of(Ki, kj[t], meanType) * area[t], dd);
                } else if (kd[t] == LK_INFILTRATION) {                       /* the surface node above (layer 1) */
                    ks = infiltration_conductance(v, c, i, j[t], (size_t)s * v.N + i, Xc, Xh, Xc[i], Hoi, v.z[i]);
                }                                                            /* a soil row has no runoff link */
                if (HEAT && (kd[t] == LK_SOIL_LAT || kd[t] == LK_SOIL_VERT))
                    add_thermal_fluxes_of(v.heat.vapor != 0, wTi, wLi, wVi, wT[t], wL[t], wV[t], area[t], d3[t], invFlux);
                k[s] = ks;
                sum += ks;
#if SF3D_ASM_SCHED_BARRIER
                if ((t + 1) % SF3D_ASM_SCHED_BARRIER == 0)
                    __builtin_amdgcn_sched_barrier(0);  /* one link's divide -> log -> divide chain at a time (every N-th link with
                                                         * -DSF3D_ASM_SCHED_BARRIER=N): the scheduler would otherwise interleave
                                                         * the five of a group and run out of registers (371 us instead of 304) */
#endif
            }
        }
        store_row<NT>(v, A2w, cd, i, k, sum, Hoi, dt, invFlux, Ci, flowi);
    }
}

/* one launch: blocks [0, nbSurf) assemble the surface rows (and reduce the Courant maximum),
 * blocks [nbSurf, nbSurf + nbSoil) the soil rows.  FUSED: the block that arrives last takes the
 * Courant decision (checkCourant) instead of a separate one-block kernel. */
template <bool FUSED, bool NT, bool HEAT>
__device__ __forceinline__ void body_assemble(const DevView& v)
{
    fm_init();
    double bm = 0.;
    if (blockIdx.x < v.nbSurf) bm = assemble_surface_rows<NT, HEAT>(v, blockIdx.x, v.nbSurf);
    else assemble_soil_rows<NT, HEAT>(v, blockIdx.x - v.nbSurf, v.nbSoil);
    if (!FUSED) {
        if (threadIdx.x == 0 && blockIdx.x < v.nbSurf) v.part0[blockIdx.x] = bm;
        return;
    }
    __syncthreads();
    if (!arrive_last(v, bm, 0., false)) return;
    double m = 0.;                                        /* soil blocks published 0: the maximum is unchanged */
    for (uint32_t k = threadIdx.x; k < gridDim.x; k += SF3D_BLOCK)
        m = dmax(m, __hip_atomic_load(&v.part0[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    double vals[3] = {block_max(m), 0., 0.};
    if (!dist_allgather(v, v.ctrl, vals, 1)) return;
    if (threadIdx.x == 0) courant_decision(v.ctrl, vals[0]);
}
template <bool FUSED, bool NT, bool HEAT>
__global__ void __launch_bounds__(SF3D_BLOCK, HEAT ? SF3D_ASM_HEAT_WAVES : SF3D_ASM_WAVES) k_assemble(DevView v)
{
    if (v.ctrl->stage != ST_APPROX) return;
    body_assemble<FUSED, NT, HEAT>(v);
}

/* ---- early Courant check (one GPU, water only) ------------------------------------------------------------------------------------
 * checkCourant (cpusolver.cpp:248-281) refuses an attempt on the Courant number of the SURFACE links alone (runoffConductance,
 * water.cpp:413-487: H, Hold, pond, roughness and - at approximation 0 - the waterFlow of the two surface nodes); the reference has
 * assembled only the surface rows by then (:412-421).  The product's k_props + k_assemble do the whole approximation (properties of
 * every node, every row: ~430 us at C4) before the decision - wasted when it is a refusal (42 of the 118 attempts of C4 F60 hour 0).
 * While the last Courant number is high (>= DevView::probeMin) and a refusal happened within the last few approximations
 * (Ctrl::probeBudget) two small launches run first: k_props_surface = updateBoundaryWaterData
 * of the surface nodes (what k_props does for them, bit for bit - it runs again in k_props), k_courant_probe = the runoff links of
 * the surface rows (assemble_surface_rows<COURANT_ONLY>: the same link_conductance calls, each link from one of its ends only - its
 * Courant term is the same number from both -, nothing stored) and, in the last block,
 * checkCourant's refusal when the
 * maximum calls for it: the same reject path, the same counters; the guarded k_props / k_assemble that follow then already work on
 * the next attempt.  When the maximum passes nothing is decided here - k_assemble's own check follows as always. */
__global__ void __launch_bounds__(SF3D_BLOCK) k_props_surface(DevView v)
{
    const Ctrl* c = v.ctrl;
    if (c->stage != ST_APPROX || !(c->courant >= v.probeMin) || (c->probeBudget == 0 && v.probeMin > 0.)) return;
    fm_init();
    const double* __restrict__ Xc = v.X[c->cur];
    const double* __restrict__ Xh = v.X[c->hold];
    FOR_EACH_CHUNK_IN(v, 0u, v.nListSurf) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (i < v.ns) boundary_update<false>(v, c, i, Xc[i], Xh[i], v.z[i], 0., 1.);
    }
}
template <bool NT>
__global__ void __launch_bounds__(SF3D_BLOCK, SF3D_ASM_WAVES) k_courant_probe(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->stage != ST_APPROX || !(c->courant >= v.probeMin) || (c->probeBudget == 0 && v.probeMin > 0.)) return;
    fm_init();
    const double bm = assemble_surface_rows<NT, false, true>(v, blockIdx.x, gridDim.x);
    __syncthreads();
    if (!arrive_last(v, bm, 0., false)) return;
    double m = 0.;
    for (uint32_t k = threadIdx.x; k < gridDim.x; k += SF3D_BLOCK)
        m = dmax(m, __hip_atomic_load(&v.part0[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    m = block_max(m);
    if (threadIdx.x == 0 && !(m < 1.01 || c->dt <= c->dtMin)) {
        /* nothing of this attempt has been stored when its first approximation is refused here: Se of the state it started from is
         * where it was (reject_attempt would point at SeHold, which approximation 0's k_props has not written) */
        const uint32_t seWas = c->seSource;
        const bool first = c->approx == 0;
        courant_decision(c, m);
        if (first) c->seSource = seWas;
        c->earlyCourant++;
    }
    else if (threadIdx.x == 0 && c->probeBudget) c->probeBudget--;      /* passed: one approximation of the budget used up */
}

#include "sf3d_cg.inc"          /* k_cg_*: preconditioned conjugate gradients standing in for the linealia hook */

/* quirk-1 compat only.  Mirrors the assembly that has just been decided into the emulated row storage of the reference
 * (computeLinearSystemElement cpusolver.cpp:348-389: every existing link writes its conductance at the running column, only a
 * non-zero one advances it; columns [1, numCols) negated, [0] = diagonal) and then does what the reference's separate
 * preconditioningMatrix pass does (:284-305) - unless the Courant check refused the attempt, in which case the reference had
 * assembled the surface rows only and left them un-normalised. */
__global__ void __launch_bounds__(SF3D_BLOCK) k_compat_rows(DevView v)
{
    Ctrl* c = v.ctrl;
    if (c->asmSeq == c->compatSeq) return;
    const bool surfOnly = c->asmSurfOnly != 0;
    constexpr uint32_t order[SF3D_SLOTS] = {0, 2, 3, 4, 5, 6, 7, 8, 9, 1};
    const size_t N = v.N;
    sf3d_d2* __restrict__ A2c = cur_A2(v);
    FOR_EACH_CHUNK_IN(v, 0u, surfOnly ? v.nListSurf : v.nList) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i) || (surfOnly && i >= v.ns)) continue;
        const ChunkDesc cd = v.cdesc[q];
        double a[SF3D_SLOTS];
        #pragma unroll
        for (int p = 0; p < SF3D_SLOTS / 2; ++p) { const sf3d_d2 t = A2c[(size_t)p * N + i]; a[2 * p] = t.x; a[2 * p + 1] = t.y; }
        const double diag = v.compatDiag[i];
        const double inv = surfOnly ? 1.0 : 1.0 / diag;
        uint32_t col = 1; bool lastDropped = false;
        #pragma unroll
        for (int o = 0; o < SF3D_SLOTS; ++o) {
            const uint32_t s = order[o];
            const bool exists = (cd.kind[s] == CK_MIXED) ? v.lkind[(size_t)s * N + i] != LK_NONE : cd.kind[s] != CK_NONE;
            if (!exists) continue;
            lastDropped = !(a[s] != 0.);                       /* a = k * -1: -0.0 for a dropped link */
            if (!lastDropped) { v.compatCv[(size_t)col * N + i] = a[s] * inv; ++col; }
        }
        if (lastDropped) v.compatCv[(size_t)col * N + i] = 0.0;   /* the conductance itself, written and never negated */
        v.compatCn[i] = (uint8_t)col;
        v.compatCv[i] = surfOnly ? diag : 1.0;
        if (!surfOnly) {
            #pragma unroll
            for (int p = 0; p < SF3D_SLOTS / 2; ++p) { sf3d_d2 t; t.x = a[2 * p] * inv; t.y = a[2 * p + 1] * inv; A2c[(size_t)p * N + i] = t; }
            v.b[i] *= inv;
        }
    }
    __syncthreads();
    if (!arrive_last(v, 0., 0., false)) return;
    if (threadIdx.x == 0) c->compatSeq = c->asmSeq;
}

/* acceptStep's link flow sums for one row (water.cpp:240-250 + updateLinkFlux :269-277): the stored, row-normalised coefficient as in
 * the reference (SURVEY.md 8a quirk 1).  A zero coefficient adds exactly 0 - unless the compat storage exists: then a dropped
 * link reads the slot after the row's last column, like getMatrixElementValue (cpusolver.h:42-52). */
template <bool NT>
__device__ __forceinline__ void accept_links_row(const DevView& v, const sf3d_d2* __restrict__ A2, uint32_t q, uint32_t i, const double* __restrict__ X, double dt)
{
    double a[SF3D_SLOTS], xj[SF3D_SLOTS], f[SF3D_SLOTS];
    uint32_t j[SF3D_SLOTS];
    #pragma unroll
    for (int p = 0; p < SF3D_SLOTS / 2; ++p) { const sf3d_d2 t = load_coeff<NT>(&A2[(size_t)p * v.N + i]); a[2 * p] = t.x; a[2 * p + 1] = t.y; }   /* non-zero only where a link exists */
    const ChunkDesc cd = v.cdesc[q];
    #pragma unroll
    for (int s = 0; s < SF3D_SLOTS; ++s) {
        if (cd.kind[s] != CK_MIXED) j[s] = i + cd.delta[s];
        else if ((cd.sweepUniform >> s) & 1u) { const uint32_t jj = i + (uint32_t)cd.delta[s]; j[s] = jj < v.N ? jj : i; }   /* a node without the link has a zero coefficient */
        else j[s] = v.lto[(size_t)s * v.N + i];
    }
    if (v.compatCv != nullptr) {
        const double stale = v.compatCv[(size_t)v.compatCn[i] * v.N + i] * v.compatCv[i];
        #pragma unroll
        for (int s = 0; s < SF3D_SLOTS; ++s) {
            const bool exists = (cd.kind[s] == CK_MIXED) ? v.lkind[(size_t)s * v.N + i] != LK_NONE : cd.kind[s] != CK_NONE;
            if (exists && !(a[s] != 0.)) a[s] = stale;
        }
    }
    const double Hi = X[i];
    #pragma unroll
    for (int s = 0; s < SF3D_SLOTS; ++s) { xj[s] = X[j[s]]; f[s] = (a[s] != 0.) ? load_stream<NT>(&v.lflowSum[(size_t)s * v.N + i]) : 0.; }
    #pragma unroll
    for (int s = 0; s < SF3D_SLOTS; ++s)
        if (a[s] != 0.) store_stream<NT>(&v.lflowSum[(size_t)s * v.N + i], f[s] + a[s] * (Hi - xj[s]) * dt);
}

/* JacobiWaterCPU, water.cpp:565-601.
 * All coefficient loads, then all neighbour gathers, are issued before the ordered accumulation
 * so that ~30 independent loads per lane are in flight (HBM-bound kernel, 152 algorithmic B/node). */
/* MODE 0: partials only (a separate k_decide_sweep follows).  MODE 1 (single GPU): the block that
 * arrives last also takes the convergence decision.  MODE 2 (multi GPU): each wave additionally puts
 * the new iterate of its boundary nodes into the neighbours' windows, and the last block all-gathers
 * the norm, copies the received halo and decides - one launch per sweep in every configuration. */
/* BND (MODE 2 only): the second half of a paired sweep on a strip (sf3d_pair.inc, DIST) - the same rows of the same sweep, but only
 * the chunks that read a neighbouring strip (DevView::bndList), from x' = X[cur] and the neighbours' x' in the window, into the
 * buffer k_sweep_pair wrote the other rows' x'' to; the norm of those other rows waits in Ctrl::pairNorm2. */
template <int MODE, bool NT, bool BND = false>
__device__ __forceinline__ void body_sweep(const DevView& v)
{
    const Ctrl* c = v.ctrl;
    const int nxt = BND ? c->pairX2 : free_buffer(c);
    const uint32_t par = c->epoch & 1u;
    const double* __restrict__ xin = v.X[c->cur];
    double* __restrict__ xout = v.X[nxt];
    const sf3d_d2* __restrict__ A2 = cur_A2(v);
    double nrm = 0., nrmLo = 0.;          /* a double-double: sf3d_physics.inc "the norm of a Jacobi sweep" */
    FOR_EACH_CHUNK_OF(BND ? v.bndList : v.chunkList, 0u, BND ? v.nBnd : v.nList) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        const bool mine = !NOT_MINE(v, i);
        double xn = 0.;
        if (mine) {
            double a[SF3D_SLOTS], xj[SF3D_SLOTS];
            uint32_t j[SF3D_SLOTS];
            #pragma unroll
            for (int p = 0; p < SF3D_SLOTS / 2; ++p) { const sf3d_d2 t = load_coeff<NT>(&A2[(size_t)p * v.N + i]); a[2 * p] = t.x; a[2 * p + 1] = t.y; }
            const ChunkDesc cd = v.cdesc[q];                                     /* wave-uniform: scalar load */
            #pragma unroll
            for (int s = 0; s < SF3D_SLOTS; ++s) {
                if (cd.kind[s] != CK_MIXED) j[s] = i + cd.delta[s];              /* offset 0 when the slot is empty */
                else if ((cd.sweepUniform >> s) & 1u) {                          /* row end: the nodes without the link have a zero coefficient */
                    const int64_t jj = (int64_t)i + cd.delta[s];
                    j[s] = (jj < 0 || jj >= (int64_t)v.N) ? i : (uint32_t)jj;
                } else j[s] = load_stream<NT>(&v.lto[(size_t)s * v.N + i]);       /* 0 for a missing link: in range */
            }
            const double bi = v.b[i], zi = v.z[i], xi = xin[i];
            #pragma unroll
            for (int s = 0; s < SF3D_SLOTS; ++s) xj[s] = xin[j[s]];
            if (MODE == 2 && v.haloDirect && cd.pad0 && (BND || c->iter > 0)) {
                /* multi GPU, second and later sweeps of an approximation: the neighbours' previous iterate sits in my window
                 * (they put it during their previous sweep, parity of the previous epoch) and has not been copied into xin -
                 * the halo copy is done once per approximation by k_post, not once per sweep on the critical path */
                const DistView* d = v.dist;
                const uint32_t parPrev = par ^ 1u;
                #pragma unroll
                for (int s = 0; s < SF3D_SLOTS; ++s) {
                    const uint32_t f = d->fsrc[(size_t)s * v.N + i];
                    if (f != SF3D_FSRC_NONE) {
                        const uint32_t p = f >> 27, k = f & 0x07FFFFFFu;
                        xj[s] = SYS_LOAD(d->payload[v.rank] + d->recvOff[p] + (size_t)(parPrev * SF3D_DIST_FIELDS + DF_X) * d->recvCount[p] + k);
                    }
                }
            }
            xn = bi;
            constexpr uint32_t order[SF3D_SLOTS] = {0, 2, 3, 4, 5, 6, 7, 8, 9, 1};
            #pragma unroll
            for (int o = 0; o < SF3D_SLOTS; ++o) {
                const uint32_t s = order[o];
                if (a[s] != 0.) xn -= a[s] * xj[s];                              /* zero entries are not in the reference's row */
            }
            if (i < v.ns) xn = dmax(xn, zi);
            double d = fabs(xn - xi);
            const double psi = fabs(xn - zi);
            if (psi > 1.) d *= (1. / psi);
            dd_add(nrm, nrmLo, d);
            xout[i] = xn;
        }
        if (MODE == 2) dist_put_chunk(v, q, lane_, par, 0, xn);
    }
    if (MODE == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      /* every wave drains its puts before the barrier */
    block_sum_dd(nrm, nrmLo);
    if (MODE == 0) {
        if (threadIdx.x == 0) { v.part0[blockIdx.x] = nrm; v.part1[blockIdx.x] = nrmLo; }
        return;
    }
    if (!arrive_last(v, nrm, nrmLo, true)) return;
    double vals[3] = {0., 0., 0.};
    sum_published_dd(v.part0, v.part1, gridDim.x, vals[0], vals[1]);
    block_sum_dd(vals[0], vals[1]);
    if (MODE == 2) {
        if (!dist_allgather(v, v.ctrl, vals, 2)) return;                  /* also the barrier that makes the neighbours' puts visible */
        if (!v.haloDirect) dist_unpack(v, par, DF_X, v.X[nxt]);           /* neighbours' new iterate on my halo */
    }
    if (BND) {
        if (threadIdx.x == 0) { Ctrl* w = v.ctrl; w->pairPending = 0; dd_merge(vals[0], vals[1], w->pairNorm2, w->pairNorm2Lo); sweep_decision(w, nxt, (vals[0] + vals[1]) / v.Nnorm); }
        return;
    }
    if (threadIdx.x == 0) { v.ctrl->singleLaunches++; sweep_decision(v.ctrl, nxt, (vals[0] + vals[1]) / v.Nnorm); }
}
template <int MODE, bool NT>
__global__ void __launch_bounds__(SF3D_BLOCK) k_sweep(DevView v)
{
    if (v.ctrl->stage != ST_SWEEP) return;
    body_sweep<MODE, NT>(v);
}
/* second iteration of a paired sweep for the rows next to a neighbouring strip: runs only when k_sweep_pair<DIST> has left its
 * first decision open (Ctrl::pairPending) */
template <bool NT>
__global__ void __launch_bounds__(SF3D_BLOCK) k_sweep_bnd(DevView v)
{
    if (v.ctrl->stage != ST_SWEEP || !v.ctrl->pairPending) return;
    body_sweep<2, NT, true>(v);
}

#include "sf3d_pair.inc"        /* k_sweep_pair: two Jacobi iterations per pass through an LDS ring */
#include "sf3d_pair_masked.inc" /* k_sweep_pair_masked: the same on layered masked grids (DEM outlines) */

/* The two sums of computeCurrentMassBalance - the storage and the sink / source term - are carried as DOUBLE-DOUBLES like the norm of a sweep
 * (sf3d_physics.inc): whichever kernel adds them, in whatever association - k_post's 2 048 blocks, k_restore, the epilogue of the resident sweep
 * loop with its own blocks, N ranks - the ONE rounding at the end gives the same double, so the balance decisions (and the storage the API
 * reports) do not depend on the launch form (round 6; rounds 1-5: plain sums in one fixed association per kernel). */
struct BalanceSums { double st = 0., stl = 0., sk = 0., skl = 0.; };
__device__ __forceinline__ void balance_terms(const DevView& v, const Ctrl* c, uint32_t i, double H, double z,
                                              double Se, BalanceSums& b)
{
    double theta;
    if (i >= v.ns) {
        const SoilDev s = v.soils[v.cls[i]];
        theta = (Se * (s.thetaS - s.thetaR)) + s.thetaR;      /* soilPhysics.cpp:38-42 */
    } else theta = dmax(H - z, 0.0);                          /* water.cpp:83 */
    dd_add(b.st, b.stl, theta * v.size[i]);
    const double fl = v.flow[i];
    if (fl != 0) dd_add(b.sk, b.skl, fl * c->dt);             /* water.cpp:136-137 */
}
/* one block's sums -> partials (separate decision kernel) or the last block's decision input: vals = (storage hi, lo, sink hi, lo) of the rank */
template <bool FUSED>
__device__ __forceinline__ bool balance_reduce(const DevView& v, BalanceSums& b, double (&vals)[4])
{
    block_sum_dd(b.st, b.stl);
    block_sum_dd(b.sk, b.skl);
    if (!FUSED) {
        if (threadIdx.x == 0) { v.part0[blockIdx.x] = b.st; v.part1[blockIdx.x] = b.stl; v.part2[blockIdx.x] = b.sk; v.part3[blockIdx.x] = b.skl; }
        return false;
    }
    if (!arrive_last4(v, b.st, b.stl, b.sk, b.skl)) return false;
    sum_published_dd(v.part0, v.part1, gridDim.x, vals[0], vals[1]);
    block_sum_dd(vals[0], vals[1]);
    sum_published_dd(v.part2, v.part3, gridDim.x, vals[2], vals[3]);
    block_sum_dd(vals[2], vals[3]);
    return true;
}

#include "sf3d_resident.inc"    /* k_sweep_resident: all iterations of an approximation in one launch, the rows resident on chip (grids that fit) */      /* (behind balance_terms: its launch also does k_post's work) */

/* cpusolver.cpp:451-457 (H = x is implicit: H is the current pool buffer) + the two sums of
 * computeCurrentMassBalance (water.cpp:71-90, 130-140) */
#ifndef SF3D_POST_WAVES
#define SF3D_POST_WAVES 8      /* 64 VGPRs: all 2 048 blocks of the grid resident at once (at 70 VGPRs 1 792 are, and the rest form a tail) */
#endif
template <bool FUSED>
__device__ __forceinline__ void body_post(const DevView& v)
{
    const Ctrl* c = v.ctrl;
    fm_init();
    const int cur = c->cur;
    const uint32_t parLastSweep = (c->epoch - 1u) & 1u;       /* the last sweep put its iterate one epoch ago */
    const bool haloLocal = c->haloLocalTag == c->epoch + 1u;   /* ... unless a paired pass with record hand-over ended on its first iterate: that halo is in the pool */
    const double* __restrict__ Xc = v.X[cur];
    BalanceSums bs;
    {   /* software-pipelined chunk loop: the loads of the next chunk (list entry, H, z, class) are issued before the two
         * pow of the current one - the kernel is latency-bound (VALU 48 % busy), three dependent round trips per chunk */
        const uint32_t lane_ = threadIdx.x & 63u;
        const uint32_t wavesTotal_ = gridDim.x * (SF3D_BLOCK / 64);
        uint32_t li_ = __builtin_amdgcn_readfirstlane(blockIdx.x * (SF3D_BLOCK / 64) + (threadIdx.x >> 6));
        uint32_t i = 0; double H = 0., z = 0.; uint16_t cl = 0; bool on = false;
        if (li_ < v.nList) {
            i = __builtin_amdgcn_readfirstlane(v.chunkList[li_]) * SF3D_CHUNK + lane_;
            on = !NOT_MINE(v, i);
            if (on) { H = Xc[i]; z = v.z[i]; cl = v.cls[i]; }
        }
        while (li_ < v.nList) {
            const uint32_t lin = li_ + wavesTotal_;
            uint32_t i2 = 0; double H2 = 0., z2 = 0.; uint16_t cl2 = 0; bool on2 = false;
            if (lin < v.nList) {
                i2 = __builtin_amdgcn_readfirstlane(v.chunkList[lin]) * SF3D_CHUNK + lane_;
                on2 = !NOT_MINE(v, i2);
                if (on2) { H2 = Xc[i2]; z2 = v.z[i2]; cl2 = v.cls[i2]; }
            }
            if (on) {
                double Se = 1.;
                if (i >= v.ns) { Se = node_se(v.soils[cl], H, z, c->wrc); v.Se[i] = Se; }
                balance_terms(v, c, i, H, z, Se, bs);
            }
            li_ = lin; i = i2; H = H2; z = z2; cl = cl2; on = on2;
        }
    }
    double vals[4];
    if (!balance_reduce<FUSED>(v, bs, vals)) return;      /* last block: evaluateWaterBalance */
    if (!dist_allgather(v, v.ctrl, vals, 3)) return;
    if (threadIdx.x == 0) {
        if (v.world > 1 && v.haloDirect && !haloLocal) {  /* the halo of the final iterate, once per approximation (k_halo_copy<1>, */
            Ctrl* w = v.ctrl;                             /* next launch): the sweeps read foreign neighbours from the window       */
            w->haloBuf = cur; w->haloPar = parLastSweep; w->haloEpoch = w->epoch;
        }
        balance_decision(v.ctrl, vals[0] + vals[1], vals[2] + vals[3]);
    }
}
template <bool FUSED>
__global__ void __launch_bounds__(SF3D_BLOCK, SF3D_POST_WAVES) k_post(DevView v)
{
    if (v.ctrl->stage != ST_POST) return;
    body_post<FUSED>(v);
}

/* restoreBestStep, water.cpp:253-267 */
template <bool FUSED, bool HEAT>
__device__ __forceinline__ void body_restore(const DevView& v)
{
    const Ctrl* c = v.ctrl;
    fm_init();
    const double* __restrict__ Xc = v.X[c->cur];
    const double* __restrict__ Xh = v.X[c->hold];
    const uint32_t par = c->epoch & 1u;
    const bool haloK = HEAT && FUSED && v.world > 1;      /* sharded heat: saveWaterFluxValues reads the neighbours' K */
    BalanceSums bs;
    FOR_EACH_CHUNK(v) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        double K = 0.;
        if (!NOT_MINE(v, i)) {
            const double H = Xc[i], Ho = Xh[i], z = v.z[i];
            double Se = 1.;
            if (i >= v.ns) {
                const SoilDev s = v.soils[v.cls[i]];
                Se = node_se(s, H, z, c->wrc);
                K = mualem_k(s, Se, c->wrc);
                if (HEAT && v.heat.vapor) {
                    const HeatDev& hv = v.heat;
                    const double Tm = (hv.TX[c->tCur][i] + hv.TX[c->tOld][i]) * 0.5;
                    K += h_isothermal_vapor_conductivity(s, Tm, H - z, h_theta_signed_psi(s, H - z, c->wrc)) * (H_G / H_RHOW);
                }
                v.Se[i] = Se; v.K[i] = K;
            }
            boundary_update<HEAT>(v, c, i, H, Ho, z, K, Se);
            balance_terms(v, c, i, H, z, Se, bs);
        }
        if (haloK) dist_put_chunk(v, q, lane_, par, DF_K, K);
    }
    if (haloK) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double vals[4];
    if (!balance_reduce<FUSED>(v, bs, vals)) return;
    if (!dist_allgather(v, v.ctrl, vals, 3)) return;
    if (haloK) dist_unpack(v, par, DF_K, v.K);
    if (threadIdx.x == 0) restore_decision(v.ctrl, vals[0] + vals[1], vals[2] + vals[3]);
}
template <bool FUSED, bool HEAT>
__global__ void __launch_bounds__(SF3D_BLOCK) k_restore(DevView v)
{
    if (v.ctrl->stage != ST_RESTORE) return;
    body_restore<FUSED, HEAT>(v);
}

/* acceptStep flow sums, water.cpp:240-250 + updateLinkFlux :269-277 */
template <bool NT>
__device__ __forceinline__ void body_accept(const DevView& v)
{
    const Ctrl* c = v.ctrl;
    const double* __restrict__ X = v.X[c->cur];
    const sf3d_d2* __restrict__ A2 = cur_A2(v);
    const double dt = c->dt;
    FOR_EACH_CHUNK(v) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i)) continue;
        accept_links_row<NT>(v, A2, q, i, X, dt);
        if (v.btype[i] != SF3D_BND_NONE) v.bflowSum[i] += v.bflowRate[i] * dt;
    }
}
template <bool NT>
__global__ void __launch_bounds__(SF3D_BLOCK) k_accept(DevView v)
{
    if (v.ctrl->stage != ST_ACCEPT) return;
    body_accept<NT>(v);
}


/* The two halves of k_accept where the link flow sums are added in batches (plain single-GPU path): the boundary sums stay in the
 * step (the next step's k_props overwrites bflowRate), and the step keeps a copy of its accepted head in the slot of the ring its
 * matrix sits in.  The link sums - read and rewrite 160 B per node to add one term each - wait: k_links_flush adds the terms of up
 * to SF3D_LINKS_RING accepted steps in one pass over the sums. */
__global__ void __launch_bounds__(SF3D_BLOCK) k_accept_boundary(DevView v)
{
    const Ctrl* c = v.ctrl;
    if (c->stage != ST_ACCEPT) return;
    const double dt = c->dt;
    const double* __restrict__ X = v.X[c->cur];
    double* __restrict__ Hk = v.Hring[c->aBuf];          /* the slot comes from the control block: the captured graphs carry no argument for it */
    FOR_EACH_CHUNK(v) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i)) continue;
        Hk[i] = X[i];
        if (v.btype[i] != SF3D_BND_NONE) v.bflowSum[i] += v.bflowRate[i] * dt;
    }
}
/* The link flow sums of the accepted steps b.slot[0 .. n), in that order: per node and slot the expression of accept_links_row applied n
 * times to a sum held in a register - the same operands in the same order, and a step whose coefficient is zero adds nothing (the sum, a
 * -0.0 included, stays what it is) - so the sums have the bits n launches of k_accept would have left.  Matrix and head of step k come
 * from slot b.slot[k] of the two rings (the pool buffer the head was accepted in is long recycled).  A sum no step touched is not stored.
 * Slots [S0, S0 + H) of a node per call: whole pairs of the matrix.  No compat rows here: where DevView::compatCv exists the sums are
 * added inside the step. */
template <bool NT, int S0, int H>
__device__ __forceinline__ void links_flush_slots(const DevView& v, const LinksBatch& b, const ChunkDesc& cd, uint32_t i)
{
    static_assert(S0 % 2 == 0 && H % 2 == 0 && S0 + H <= SF3D_SLOTS, "whole (2p, 2p+1) pairs of A2x");
    uint32_t j[H];
    double f[H];
    uint32_t touched = 0u;
    #pragma unroll
    for (int t = 0; t < H; ++t) {
        const int s = S0 + t;
        if (cd.kind[s] != CK_MIXED) j[t] = i + cd.delta[s];
        else if ((cd.sweepUniform >> s) & 1u) { const uint32_t jj = i + (uint32_t)cd.delta[s]; j[t] = jj < v.N ? jj : i; }   /* a node without the link has a zero coefficient */
        else j[t] = v.lto[(size_t)s * v.N + i];
        f[t] = load_stream<NT>(&v.lflowSum[(size_t)s * v.N + i]);
    }
    for (uint32_t k = 0; k < b.n; ++k) {
        const sf3d_d2* __restrict__ A2 = v.A2x[b.slot[k]];
        const double* __restrict__ X = v.Hring[b.slot[k]];
        const double dt = b.dt[k];
        double a[H], xj[H];
        #pragma unroll
        for (int p = 0; p < H / 2; ++p) { const sf3d_d2 t2 = load_coeff<NT>(&A2[(size_t)(S0 / 2 + p) * v.N + i]); a[2 * p] = t2.x; a[2 * p + 1] = t2.y; }   /* non-zero only where a link exists */
        const double Hi = X[i];
        #pragma unroll
        for (int t = 0; t < H; ++t) xj[t] = X[j[t]];
        #pragma unroll
        for (int t = 0; t < H; ++t)
            if (a[t] != 0.) { f[t] = f[t] + a[t] * (Hi - xj[t]) * dt; touched |= 1u << t; }
    }
    #pragma unroll
    for (int t = 0; t < H; ++t)
        if ((touched >> t) & 1u) store_stream<NT>(&v.lflowSum[(size_t)(S0 + t) * v.N + i], f[t]);
}
/* the ten slots in two groups, 4 + 6: all ten sums, coefficients, neighbour heads and indices across the loop over the steps take 108 VGPRs
 * (4 waves per SIMD; held to 96 they spill), a group of six stays below the 88 of k_accept (5 waves).  The second group reads the
 * node's own head again: 8 B of the 168 B a step costs per node, and from the cache */
template <bool NT>
__global__ void __launch_bounds__(SF3D_BLOCK) k_links_flush(DevView v, LinksBatch b)
{
    FOR_EACH_CHUNK(v) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i)) continue;
        const ChunkDesc cd = v.cdesc[q];
        links_flush_slots<NT, 0, 4>(v, b, cd, i);
        links_flush_slots<NT, 4, SF3D_SLOTS - 4>(v, b, cd, i);
    }
}

/* computeTotalWaterContent on the stored state (getTotalWaterContent / initializeBalance) */
__global__ void __launch_bounds__(SF3D_BLOCK) k_storage(DevView v)
{
    const Ctrl* c = v.ctrl;
    const double* __restrict__ Xc = v.X[c->cur];
    double st = 0.;
    FOR_EACH_CHUNK(v) {
        const uint32_t i = q * SF3D_CHUNK + lane_;
        if (NOT_MINE(v, i)) continue;
        const double H = Xc[i], z = v.z[i];
        double theta;
        if (i >= v.ns) { const SoilDev s = v.soils[v.cls[i]]; theta = (v.Se[i] * (s.thetaS - s.thetaR)) + s.thetaR; }
        else theta = dmax(H - z, 0.0);
        st += theta * v.size[i];
    }
    const double a = block_sum(st);
    if (threadIdx.x == 0) v.part0[blockIdx.x] = a;
}

