# TMVBHip.jl -- ccall shim: TopicModelsVB.jl's `@gpu train!` on libtmvb_hip.so (MI355X / gfx950).
#
# Drop this file into src/ and `include("TMVBHip.jl")` after gpuCTPF.jl (src/TopicModelsVB.jl:28); `gpu_macro.jl`
# (same directory) replaces `macro gpu` (src/macros.jl:106-284).  The shim keeps the package's surface:
#   * hipLDA / hipCTM / hipCTPF <: TopicModel carry the fields that `@gpu`, `predict`, `topicdist`, `showtopics` read
#     (src/gpuLDA.jl:6-21, src/gpuCTM.jl:6-24, src/gpuCTPF.jl:6-46);
#   * one Julia function per device operator, as the reference has (src/gpuLDA.jl:132-340, src/gpuCTM.jl:166-480,
#     src/gpuCTPF.jl:314-670) -- the per-document operator chain of a sweep is ONE fused kernel here, so
#     update_phi!/update_gamma!/update_Elogtheta! (LDA), update_phi!/update_logzeta!/update_vsq!/update_lambda! (CTM) and
#     update_xi!/update_phi!/update_zayin!/update_gimel! (CTPF) are reached through `update_estep!`;
#   * train! has the signatures and defaults of src/gpuLDA.jl:347, src/gpuCTM.jl:487, src/gpuCTPF.jl:677; argument errors
#     are ArgumentError, state errors TopicModelError, corpus errors CorpusError, with the reference's messages;
#   * predict / topicdist methods for the hip types (src/modelutils.jl:831-913, :946-970); gendoc / gencorp (:594-649) on the device;
#   * NEW: document-sharded multi-GPU train! behind the same call -- `hipComm` wraps the library's communicator (RCCL
#     over xGMI, or a host all-reduce callback), `train!(::Vector{hipLDA})` drives n GPUs from one host thread.
#
# NOTE: Julia is not installed in the build image of this repository, so this file has not been executed there.  Every
# ccall below is checked against include/tmvb.h by tests/test_julia_shim_static.py (name, arity, argument classes), and
# every call sequence is mirrored -- and tested on the GPU -- by the Python host in topicmodelsvb.jl_amd/*.py through
# the same C ABI.

const LIBTMVB = get(ENV, "TMVB_HIP_LIB", "libtmvb_hip.so")
# eight hardware queues for the process's HIP streams, before the runtime initialises (the library's constructor does the same: tmvb_core.hip)
haskey(ENV, "GPU_MAX_HW_QUEUES") || (ENV["GPU_MAX_HW_QUEUES"] = "8")

const TMVB_OK, TMVB_EINVAL, TMVB_ESHAPE, TMVB_ECORPUS, TMVB_ENOMEM, TMVB_EHIP, TMVB_ENONFINITE, TMVB_ENODEVICE, TMVB_ERCCL = 0, 1, 2, 3, 4, 5, 6, 7, 8
const TMVB_UNIQUE_ID_BYTES = 128

function tmvb_check(rc::Integer)
	rc == TMVB_OK && return nothing
	msg = unsafe_string(ccall((:tmvb_last_error, LIBTMVB), Cstring, ()))
	rc == TMVB_EINVAL     && throw(ArgumentError(msg))
	rc == TMVB_ESHAPE     && throw(TopicModelError(msg))
	rc == TMVB_ENONFINITE && throw(TopicModelError(msg))
	rc == TMVB_ECORPUS    && throw(CorpusError(msg))
	rc == TMVB_ENOMEM     && throw(OutOfMemoryError())
	error("libtmvb_hip (status $rc): " * msg)
end

# ---------------------------------------------------------------------------------------------- context and corpus

"cl.create_compute_context() (src/gpuLDA.jl:64): one GPU + one in-order stream."
function tmvb_context(device::Integer)
	ctx = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_ctx_create, LIBTMVB), Cint, (Int32, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), device, C_NULL, ctx))
	return ctx[]
end

"Corpus half of update_buffer! (src/modelutils.jl:370-388, :438-472): flat 0-based CSR."
function tmvb_upload_corpus(ctx::Ptr{Cvoid}, corp::Corpus)
	M, V, U = size(corp)
	doc_ptr = Int64[0; cumsum([length(doc.terms) for doc in corp])]
	terms   = Int32.(reduce(vcat, [doc.terms for doc in corp]; init=Int[]) .- 1)
	counts  = Int32.(reduce(vcat, [doc.counts for doc in corp]; init=Int[]))
	rdr_ptr = Int64[0; cumsum([length(doc.readers) for doc in corp])]
	readers = Int32.(reduce(vcat, [doc.readers for doc in corp]; init=Int[]) .- 1)
	ratings = Int32.(reduce(vcat, [doc.ratings for doc in corp]; init=Int[]))
	h = Ref{Ptr{Cvoid}}(C_NULL)
	GC.@preserve doc_ptr terms counts rdr_ptr readers ratings begin
		tmvb_check(ccall((:tmvb_corpus_create, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ref{Ptr{Cvoid}}),
			ctx, M, V, U, doc_ptr, terms, counts, U > 0 ? pointer(rdr_ptr) : C_NULL,
			U > 0 ? pointer(readers) : C_NULL, U > 0 ? pointer(ratings) : C_NULL, h))
	end
	return h[]
end

tmvb_destroy_corpus(dcorp::Ptr{Cvoid}) = ccall((:tmvb_corpus_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), dcorp)
tmvb_destroy_context(ctx::Ptr{Cvoid}) = ccall((:tmvb_ctx_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), ctx)

# model.topics = [reverse(sortperm(vec(B[i,:]))) for i in 1:K] (src/gpuLDA.jl:374 and its siblings) as ONE stable segmented sort on the device,
# read backwards (tmvb_topic_order): K = 50 sorts of V = 25 319 values one after the other were the largest host item of a train! call.
function hip_topics(ctx::Ptr{Cvoid}, B::Matrix{Float64})
	K, V = size(B)
	out = Matrix{Int32}(undef, V, K)                 # the library's row-major [K][V] is this column-major V x K
	tmvb_check(ccall((:tmvb_topic_order, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int64, Ptr{Int32}), ctx, B, K, V, out))
	[Int.(out[:, i]) for i in 1:K]
end

cols(m::Matrix{Float64}) = [m[:,d] for d in 1:size(m, 2)]
checkelbo_arg(checkelbo::Real) = checkelbo == Inf ? Int32(0) : Int32(checkelbo)

function check_train_args(tols, iters, checkelbo)
	all(tols .>= 0)														|| throw(ArgumentError("tolerance parameters must be nonnegative."))
	all(iters .>= 0)													|| throw(ArgumentError("iteration parameters must be nonnegative."))
	(isa(checkelbo, Integer) & (checkelbo > 0)) | (checkelbo == Inf)	|| throw(ArgumentError("checkelbo parameter must be a positive integer or Inf."))
end

"The printing half of check_elbo! (src/modelutils.jl:578-579); the first delta refers to the ELBO evaluated before the first iteration."
function print_delbo(traj::Vector{Float64}, done::Integer, baseline::Float64)
	prev = baseline
	for k in 1:done
		isnan(traj[k]) && continue
		println(k, " ∆elbo: ", round(traj[k] - prev, digits=3))
		prev = traj[k]
	end
end

# ---------------------------------------------------------------------------------------------- communicator (new)
# Document-sharded runs: every GPU holds a contiguous document shard; ONE all-reduce of the packed sufficient statistics
# per outer iteration happens inside the library (include/tmvb.h, "communicator").

mutable struct hipComm
	handle::Ptr{Cvoid}
	keep::Any                       # the @cfunction closure of a host transport must outlive the communicator
end

"128 bytes that rank 0 hands to every other rank (MPI.bcast, Distributed.jl, a file ...)."
function tmvb_unique_id()
	id = zeros(UInt8, TMVB_UNIQUE_ID_BYTES)
	tmvb_check(ccall((:tmvb_comm_unique_id, LIBTMVB), Cint, (Ptr{UInt8},), id))
	return id
end

"One process per GPU: ncclCommInitRank inside the library."
function hipComm(ctx::Ptr{Cvoid}, unique_id::Vector{UInt8}, nranks::Integer, rank::Integer)
	length(unique_id) == TMVB_UNIQUE_ID_BYTES || throw(ArgumentError("unique id must be $TMVB_UNIQUE_ID_BYTES bytes."))
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_comm_create_rccl, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32, Ref{Ptr{Cvoid}}), ctx, unique_id, nranks, rank, h))
	return finalizer(c -> ccall((:tmvb_comm_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), c.handle), hipComm(h[], nothing))
end

"One host thread, n GPUs: ncclCommInitAll over the contexts of the given models."
function hipComms(ctxs::Vector{Ptr{Cvoid}})
	out = fill(C_NULL, length(ctxs))
	tmvb_check(ccall((:tmvb_comm_create_rccl_all, LIBTMVB), Cint, (Ptr{Ptr{Cvoid}}, Int32, Ptr{Ptr{Cvoid}}), ctxs, length(ctxs), out))
	return [finalizer(c -> ccall((:tmvb_comm_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), c.handle), hipComm(h, nothing)) for h in out]
end

"""
Host transport: `allreduce!(buf)` must leave the element-wise sum over all ranks in `buf` (a Vector{Float32} or
Vector{Float64} view of pinned host memory), e.g. `buf -> MPI.Allreduce!(buf, +, comm)`.
"""
function hipComm(ctx::Ptr{Cvoid}, allreduce!::Function, nranks::Integer, rank::Integer)
	function tramp(user::Ptr{Cvoid}, buf::Ptr{Cvoid}, count::Int64, dtype::Int32)::Cint
		try
			T = dtype == 0 ? Float32 : Float64
			allreduce!(unsafe_wrap(Array, Ptr{T}(buf), count))
			return Cint(0)
		catch
			return Cint(1)
		end
	end
	cb = @cfunction($tramp, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int32))
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_comm_create_host, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}), ctx, nranks, rank, cb, C_NULL, h))
	return finalizer(c -> ccall((:tmvb_comm_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), c.handle), hipComm(h[], cb))
end

# ---------------------------------------------------------------------------------------------- LDA

mutable struct hipLDA <: TopicModel
	K::Int
	M::Int
	V::Int
	N::Vector{Int}
	C::Vector{Int}
	corp::Corpus
	topics::VectorList{Int}
	alpha::Vector{Float64}
	beta::Matrix{Float64}
	beta_old::Matrix{Float64}
	Elogtheta::VectorList{Float64}
	Elogtheta_old::VectorList{Float64}
	gamma::VectorList{Float64}
	elbo::Float64
	ctx::Ptr{Cvoid}
	dcorp::Ptr{Cvoid}
	handle::Ptr{Cvoid}
	comm::Union{hipComm, Nothing}
end

"gpuLDA(corp, K) (src/gpuLDA.jl:45-84), built from the host model whose state it takes over (src/macros.jl:113-134)."
function hipLDA(model::LDA; device::Integer=0)
	ctx = tmvb_context(device)
	dcorp = tmvb_upload_corpus(ctx, model.corp)
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_lda_create, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), ctx, dcorp, model.K, h))
	m = hipLDA(model.K, model.M, model.V, model.N, model.C, model.corp, model.topics, model.alpha, model.beta,
		model.beta_old, model.Elogtheta, model.Elogtheta_old, model.gamma, model.elbo, ctx, dcorp, h[], nothing)
	finalizer(m) do x
		ccall((:tmvb_lda_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), x.handle)
		tmvb_destroy_corpus(x.dcorp)
		tmvb_destroy_context(x.ctx)
	end
	return m
end

"State half of update_buffer! (src/modelutils.jl:390-396)."
function update_buffer!(model::hipLDA)
	beta, beta_old = Matrix{Float64}(model.beta), Matrix{Float64}(model.beta_old)   # column-major K x V
	gamma, El, Elo = hcat(model.gamma...), hcat(model.Elogtheta...), hcat(model.Elogtheta_old...)
	elbo = Ref{Float64}(model.elbo)
	GC.@preserve beta beta_old gamma El Elo begin
		tmvb_check(ccall((:tmvb_lda_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
			model.handle, model.alpha, beta, beta_old, gamma, El, Elo, elbo))
	end
end

"update_host! (src/modelutils.jl:501-516); phi is never materialised."
function update_host!(model::hipLDA)
	K, M, V = model.K, model.M, model.V
	alpha = zeros(K); beta = zeros(K, V); beta_old = zeros(K, V)
	gamma = zeros(K, M); El = zeros(K, M); Elo = zeros(K, M); elbo = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_lda_get_state, LIBTMVB), Cint,
		(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
		model.handle, alpha, beta, beta_old, gamma, El, Elo, elbo))
	model.alpha, model.beta, model.beta_old = alpha, beta, beta_old
	model.gamma, model.Elogtheta, model.Elogtheta_old = cols(gamma), cols(El), cols(Elo)
	model.elbo = elbo[]
end

# one Julia function per device operator, as in src/gpuLDA.jl:132-340
"update_phi! / update_gamma! / update_Elogtheta! sweeps + update_beta!(model, d) of every document (src/LDA.jl:170-180)."
update_estep!(model::hipLDA, viter::Integer, vtol::Real) = tmvb_check(ccall((:tmvb_lda_estep, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), model.handle, viter, vtol))
update_Elogtheta_sum!(model::hipLDA) = tmvb_check(ccall((:tmvb_lda_reduce_docs, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
"Sharded run (set_comm!): update_estep! + update_Elogtheta_sum! + the statistics all-reduce, issued in vocabulary slabs under the last statistics pass."
update_estep_allreduce!(model::hipLDA, viter::Integer, vtol::Real) = tmvb_check(ccall((:tmvb_lda_estep_allreduce, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), model.handle, viter, vtol))
update_beta!(model::hipLDA) = tmvb_check(ccall((:tmvb_lda_update_beta, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
update_alpha!(model::hipLDA, niter::Integer, ntol::Real) = tmvb_check(ccall((:tmvb_lda_update_alpha, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), model.handle, niter, ntol))
function update_elbo!(model::hipLDA)
	e = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_lda_update_elbo, LIBTMVB), Cint, (Ptr{Cvoid}, Ref{Float64}), model.handle, e))
	model.elbo = e[]
end

"Attach a communicator: this model's corpus is one document shard of a corpus of M_total documents."
function set_comm!(model::hipLDA, comm::Union{hipComm, Nothing}, M_total::Integer)
	tmvb_check(ccall((:tmvb_lda_set_comm, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), model.handle, comm === nothing ? C_NULL : comm.handle, M_total))
	model.comm = comm
	nothing
end

"""
    train!(model::hipLDA; iter=150, tol=1.0, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2, checkelbo=1, printelbo=true)

Same signature as train!(::gpuLDA) (src/gpuLDA.jl:347-376), semantics of the CPU path (src/LDA.jl:161-187: per-document
exit rule :175).  With a communicator attached every rank calls it with the same arguments (document-sharded train!).
"""
function train!(model::hipLDA; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/model.K^2, viter::Integer=10, vtol::Real=1/model.K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	update_buffer!(model)
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(model.elbo)
	tmvb_check(ccall((:tmvb_lda_train, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		model.handle, iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	(iter > 0) && update_host!(model)
	model.topics = hip_topics(model.ctx, model.beta)                             # reverse(sortperm(.)) per topic
	nothing
end

"""
    train_stochastic!(model::hipLDA; batch=4096, epochs=2, tau0=1.0, kappa=0.7, order=nothing, final_pass=true, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2)

Minibatch training (stepwise EM; include/tmvb.h, "stochastic (minibatch) training"): the loop body of train! (src/LDA.jl:170-182) once per batch of
`batch` documents (equal cuts, a ragged last one), alpha and beta moving after every batch with rho_t = (tau0 + t)^(-kappa).  `order` (0-based batch ids,
repeats allowed) replaces the default of `epochs` passes in corpus order: the library draws no random number, a shuffled order comes from the host.
Takes the model's state over like train!, and leaves gamma / Elogtheta of every document under the final alpha, beta when `final_pass`.
Returns (Sbar, Ebar, t): the running statistic (K x V), its tail and the step counter.
"""
function train_stochastic!(model::hipLDA; batch::Integer=4096, epochs::Integer=2, tau0::Real=1.0, kappa::Real=0.7, order::Union{Nothing, Vector{<:Integer}}=nothing,
		final_pass::Bool=true, niter::Integer=1000, ntol::Real=1/model.K^2, viter::Integer=10, vtol::Real=1/model.K^2)
	check_train_args([ntol, vtol], [niter, viter], Inf)
	batch >= 1						|| throw(ArgumentError("batch parameter must be a positive integer."))
	epochs >= 0						|| throw(ArgumentError("epochs parameter must be a nonnegative integer."))
	(isfinite(tau0) & (tau0 >= 0))	|| throw(ArgumentError("tau0 parameter must be nonnegative."))
	(0.5 < kappa <= 1)				|| throw(ArgumentError("kappa parameter must be in (0.5, 1]."))
	K, M, V = model.K, model.M, model.V
	cuts = Int64[collect(0:batch:M-1); M]
	B = length(cuts) - 1
	steps = Int32.(order === nothing ? repeat(collect(0:B-1), epochs) : order)
	doc_ptr = Int64[0; cumsum([length(doc.terms) for doc in model.corp])]
	terms   = Int32.(reduce(vcat, [doc.terms for doc in model.corp]; init=Int[]) .- 1)
	counts  = Int32.(reduce(vcat, [doc.counts for doc in model.corp]; init=Int[]))
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_lda_svi_create, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int64}, Int32, Ref{Ptr{Cvoid}}),
		model.ctx, M, V, doc_ptr, terms, counts, K, cuts, B, h))
	sbar = zeros(K, V); ebar = zeros(K); t = Ref{Int64}(0)
	try
		beta, beta_old = Matrix{Float64}(model.beta), Matrix{Float64}(model.beta_old)
		gamma, El = hcat(model.gamma...), hcat(model.Elogtheta...)
		tmvb_check(ccall((:tmvb_lda_svi_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
			h[], model.alpha, beta, beta_old, gamma, El, C_NULL, C_NULL, C_NULL))
		tmvb_check(ccall((:tmvb_lda_svi_set_schedule, LIBTMVB), Cint, (Ptr{Cvoid}, Float64, Float64), h[], tau0, kappa))
		tmvb_check(ccall((:tmvb_lda_svi_run, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Float64, Int32, Float64),
			h[], steps, length(steps), niter, ntol, viter, vtol))
		final_pass && tmvb_check(ccall((:tmvb_lda_svi_final_pass, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), h[], viter, vtol))
		alpha = zeros(K); beta = zeros(K, V); beta_old = zeros(K, V); gamma = zeros(K, M); El = zeros(K, M)
		tmvb_check(ccall((:tmvb_lda_svi_get_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
			h[], alpha, beta, beta_old, gamma, El, sbar, ebar, t))
		model.alpha, model.beta, model.beta_old = alpha, beta, beta_old
		model.gamma, model.Elogtheta, model.Elogtheta_old = cols(gamma), cols(El), cols(El)
	finally
		ccall((:tmvb_lda_svi_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), h[])
	end
	update_buffer!(model)                                                        # the resident handle follows: predict / update_elbo! see the trained state
	model.topics = hip_topics(model.ctx, model.beta)
	return sbar, ebar, t[]
end

"""
    train!(models::Vector{hipLDA}; kwargs...)

One host thread, n GPUs: models[i] holds the i-th document shard on device i and the i-th communicator of
`hipComms([m.ctx for m in models])` (attach with set_comm!).  The n all-reduces of an iteration form one RCCL group.
"""
function train!(models::Vector{hipLDA}; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/models[1].K^2, viter::Integer=10, vtol::Real=1/models[1].K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	foreach(update_buffer!, models)
	hs = Ptr{Cvoid}[m.handle for m in models]
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(models[1].elbo)
	tmvb_check(ccall((:tmvb_lda_train_group, LIBTMVB), Cint,
		(Ptr{Ptr{Cvoid}}, Int32, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		hs, length(hs), iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	for m in models
		(iter > 0) && update_host!(m)
		m.topics = hip_topics(m.ctx, m.beta)
	end
	nothing
end

"predict (src/modelutils.jl:831-855) on the device: the fused E-step with the trained alpha / beta frozen, no M-step."
function predict(corp::Corpus, train_model::hipLDA; iter::Integer=10, tol::Real=1/train_model.K^2)
	check_corp(corp)
	(corp.vocab == train_model.corp.vocab)	|| throw(CorpusError("predict corpus and train_model corpus must have identical vocabularies."))
	(tol >= 0)								|| throw(ArgumentError("tolerance parameter must be nonnegative."))
	(iter >= 0)								|| throw(ArgumentError("iteration parameter must be nonnegative."))
	host = LDA(corp, train_model.K)
	host.alpha, host.beta, host.beta_old, host.topics = train_model.alpha, train_model.beta, copy(train_model.beta), train_model.topics
	dev = hipLDA(host)
	update_buffer!(dev)
	update_estep!(dev, iter, tol)
	update_host!(dev)
	host.gamma, host.Elogtheta, host.Elogtheta_old = dev.gamma, dev.Elogtheta, dev.Elogtheta_old
	return host
end

function topicdist(model::hipLDA, d::Integer)       # src/modelutils.jl:946-951
	(d <= length(model.corp)) || throw(CorpusError("document index outside corpus range."))
	return model.gamma[d] / sum(model.gamma[d])
end

# ---------------------------------------------------------------------------------------------- CTM
# gpuCTM replacement (src/gpuCTM.jl:6-98).

mutable struct hipCTM <: TopicModel
	K::Int; M::Int; V::Int; N::Vector{Int}; C::Vector{Int}
	corp::Corpus; topics::VectorList{Int}
	mu::Vector{Float64}; sigma::Matrix{Float64}; invsigma::Matrix{Float64}
	beta::Matrix{Float64}; beta_old::Matrix{Float64}
	lambda::VectorList{Float64}; lambda_old::VectorList{Float64}; vsq::VectorList{Float64}; logzeta::Vector{Float64}
	elbo::Float64
	ctx::Ptr{Cvoid}; dcorp::Ptr{Cvoid}; handle::Ptr{Cvoid}
	comm::Union{hipComm, Nothing}
end

function hipCTM(model::CTM; device::Integer=0)
	ctx = tmvb_context(device)
	dcorp = tmvb_upload_corpus(ctx, model.corp)
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_ctm_create, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), ctx, dcorp, model.K, h))
	m = hipCTM(model.K, model.M, model.V, model.N, model.C, model.corp, model.topics, model.mu, Matrix(model.sigma),
		Matrix(model.invsigma), model.beta, model.beta_old, model.lambda, model.lambda_old, model.vsq, model.logzeta,
		model.elbo, ctx, dcorp, h[], nothing)
	finalizer(m) do x
		ccall((:tmvb_ctm_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), x.handle)
		tmvb_destroy_corpus(x.dcorp)
		tmvb_destroy_context(x.ctx)
	end
	return m
end

"update_buffer! (src/modelutils.jl:400-436): beta_old / lambda_old travel too (update_elbo! rebuilds phi from them, src/CTM.jl:93)."
function update_buffer!(model::hipCTM)
	beta, beta_old = Matrix{Float64}(model.beta), Matrix{Float64}(model.beta_old)
	lam, lam_old, vsq = hcat(model.lambda...), hcat(model.lambda_old...), hcat(model.vsq...)
	elbo = Ref{Float64}(model.elbo)
	GC.@preserve beta beta_old lam lam_old vsq begin
		tmvb_check(ccall((:tmvb_ctm_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
			model.handle, model.mu, model.sigma, model.invsigma, beta, beta_old, lam, lam_old, vsq, model.logzeta, elbo))
	end
end

function update_host!(model::hipCTM)        # src/modelutils.jl:519-537
	K, M, V = model.K, model.M, model.V
	mu = zeros(K); sg = zeros(K, K); isg = zeros(K, K); beta = zeros(K, V); beta_old = zeros(K, V)
	lam = zeros(K, M); lam_old = zeros(K, M); vsq = zeros(K, M); lz = zeros(M); elbo = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_ctm_get_state, LIBTMVB), Cint,
		(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
		model.handle, mu, sg, isg, beta, beta_old, lam, lam_old, vsq, lz, elbo))
	model.mu, model.sigma, model.invsigma, model.beta, model.beta_old = mu, sg, isg, beta, beta_old
	model.lambda, model.lambda_old, model.vsq = cols(lam), cols(lam_old), cols(vsq)
	model.logzeta = lz; model.elbo = elbo[]
end

# one Julia function per device operator (src/gpuCTM.jl:166-480)
"update_phi! / update_logzeta! / update_vsq! / update_lambda! sweeps + update_beta!(model, d) of every document (src/CTM.jl:194-205)."
update_estep!(model::hipCTM, niter::Integer, ntol::Real, viter::Integer, vtol::Real) = tmvb_check(ccall((:tmvb_ctm_estep, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64, Int32, Float64), model.handle, niter, ntol, viter, vtol))
"sum_d lambda_d, sum_d vsq_d and the MFMA scatter matrix with the current (= previous) mu."
update_doc_sums!(model::hipCTM) = tmvb_check(ccall((:tmvb_ctm_reduce_docs, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
update_beta!(model::hipCTM) = tmvb_check(ccall((:tmvb_ctm_update_beta, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))      # src/gpuCTM.jl:253
update_sigma!(model::hipCTM) = tmvb_check(ccall((:tmvb_ctm_update_sigma, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))    # :200 -- before update_mu! (quirk Q2)
update_mu!(model::hipCTM) = tmvb_check(ccall((:tmvb_ctm_update_mu, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))          # :166
function update_elbo!(model::hipCTM)
	e = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_ctm_update_elbo, LIBTMVB), Cint, (Ptr{Cvoid}, Ref{Float64}), model.handle, e))
	model.elbo = e[]
end

function set_comm!(model::hipCTM, comm::Union{hipComm, Nothing}, M_total::Integer)
	tmvb_check(ccall((:tmvb_ctm_set_comm, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), model.handle, comm === nothing ? C_NULL : comm.handle, M_total))
	model.comm = comm
	nothing
end

"""
    train!(model::hipCTM; iter=150, tol=1.0, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2, checkelbo=1, printelbo=true)

Signature of train!(::gpuCTM) (src/gpuCTM.jl:487-519), semantics of the CPU path (src/CTM.jl:185-213).
"""
function train!(model::hipCTM; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/model.K^2, viter::Integer=10, vtol::Real=1/model.K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	update_buffer!(model)
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(model.elbo)
	tmvb_check(ccall((:tmvb_ctm_train, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		model.handle, iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	(iter > 0) && update_host!(model)
	model.topics = hip_topics(model.ctx, model.beta)                             # reverse(sortperm(.)) per topic
	nothing
end

"""
    train_stochastic!(model::hipCTM; batch=4096, epochs=2, tau0=1.0, kappa=0.7, order=nothing, final_pass=true, niter=1000, ntol=1/K^2, viter=10, vtol=1/K^2)

Minibatch training (stepwise EM; include/tmvb.h, "stochastic (minibatch) training for CTM"): the loop body of train! (src/CTM.jl:194-208) once per batch
of `batch` documents (equal cuts, a ragged last one), mu, sigma and beta moving after every batch with rho_t = (tau0 + t)^(-kappa).  `order` (0-based batch
ids, repeats allowed) replaces the default of `epochs` passes in corpus order: the library draws no random number, a shuffled order comes from the host.
Takes the model's state over like train!, and leaves lambda / vsq / logzeta of every document under the final globals when `final_pass`.
Returns (Sbar, lbar, vbar, Cbar, mref, t): the running statistic (K x V), its tail about mref, and the step counter.
"""
function train_stochastic!(model::hipCTM; batch::Integer=4096, epochs::Integer=2, tau0::Real=1.0, kappa::Real=0.7, order::Union{Nothing, Vector{<:Integer}}=nothing,
		final_pass::Bool=true, niter::Integer=1000, ntol::Real=1/model.K^2, viter::Integer=10, vtol::Real=1/model.K^2)
	check_train_args([ntol, vtol], [niter, viter], Inf)
	batch >= 1						|| throw(ArgumentError("batch parameter must be a positive integer."))
	epochs >= 0						|| throw(ArgumentError("epochs parameter must be a nonnegative integer."))
	(isfinite(tau0) & (tau0 >= 0))	|| throw(ArgumentError("tau0 parameter must be nonnegative."))
	(0.5 < kappa <= 1)				|| throw(ArgumentError("kappa parameter must be in (0.5, 1]."))
	K, M, V = model.K, model.M, model.V
	cuts = Int64[collect(0:batch:M-1); M]
	B = length(cuts) - 1
	steps = Int32.(order === nothing ? repeat(collect(0:B-1), epochs) : order)
	doc_ptr = Int64[0; cumsum([length(doc.terms) for doc in model.corp])]
	terms   = Int32.(reduce(vcat, [doc.terms for doc in model.corp]; init=Int[]) .- 1)
	counts  = Int32.(reduce(vcat, [doc.counts for doc in model.corp]; init=Int[]))
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_ctm_svi_create, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int64}, Int32, Ref{Ptr{Cvoid}}),
		model.ctx, M, V, doc_ptr, terms, counts, K, cuts, B, h))
	sbar = zeros(K, V); lbar = zeros(K); vbar = zeros(K); cbar = zeros(K, K); mref = zeros(K); t = Ref{Int64}(0)
	try
		beta, beta_old = Matrix{Float64}(model.beta), Matrix{Float64}(model.beta_old)
		lam, vsq = hcat(model.lambda...), hcat(model.vsq...)
		tmvb_check(ccall((:tmvb_ctm_svi_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
			 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
			h[], model.mu, model.sigma, model.invsigma, beta, beta_old, lam, vsq, model.logzeta, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
		tmvb_check(ccall((:tmvb_ctm_svi_set_schedule, LIBTMVB), Cint, (Ptr{Cvoid}, Float64, Float64), h[], tau0, kappa))
		tmvb_check(ccall((:tmvb_ctm_svi_run, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Int64, Int32, Float64, Int32, Float64),
			h[], steps, length(steps), niter, ntol, viter, vtol))
		final_pass && tmvb_check(ccall((:tmvb_ctm_svi_final_pass, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64, Int32, Float64), h[], niter, ntol, viter, vtol))
		mu = zeros(K); sg = zeros(K, K); isg = zeros(K, K); beta = zeros(K, V); beta_old = zeros(K, V)
		lam = zeros(K, M); vsq = zeros(K, M); lz = zeros(M)
		tmvb_check(ccall((:tmvb_ctm_svi_get_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
			 Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}),
			h[], mu, sg, isg, beta, beta_old, lam, vsq, lz, sbar, lbar, vbar, cbar, mref, t))
		model.mu, model.sigma, model.invsigma, model.beta, model.beta_old = mu, sg, isg, beta, beta_old
		model.lambda, model.lambda_old, model.vsq, model.logzeta = cols(lam), cols(lam), cols(vsq), lz
	finally
		ccall((:tmvb_ctm_svi_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), h[])
	end
	update_buffer!(model)                                                        # the resident handle follows: predict / update_elbo! see the trained state
	model.topics = hip_topics(model.ctx, model.beta)
	return sbar, lbar, vbar, cbar, mref, t[]
end

function train!(models::Vector{hipCTM}; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/models[1].K^2, viter::Integer=10, vtol::Real=1/models[1].K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	foreach(update_buffer!, models)
	hs = Ptr{Cvoid}[m.handle for m in models]
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(models[1].elbo)
	tmvb_check(ccall((:tmvb_ctm_train_group, LIBTMVB), Cint,
		(Ptr{Ptr{Cvoid}}, Int32, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		hs, length(hs), iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	for m in models
		(iter > 0) && update_host!(m)
		m.topics = hip_topics(m.ctx, m.beta)
	end
	nothing
end

"predict (src/modelutils.jl:886-913) on the device: the fused CTM E-step with mu / sigma / beta frozen."
function predict(corp::Corpus, train_model::hipCTM; iter::Integer=10, tol::Real=1/train_model.K^2, niter::Integer=1000, ntol::Real=1/train_model.K^2)
	check_corp(corp)
	(corp.vocab == train_model.corp.vocab)	|| throw(CorpusError("predict corpus and train_model corpus must have identical vocabularies."))
	all([tol, ntol] .>= 0)					|| throw(ArgumentError("tolerance parameters must be nonnegative."))
	all([iter, niter] .>= 0)				|| throw(ArgumentError("iteration parameters must be nonnegative."))
	host = CTM(corp, train_model.K)
	host.mu, host.sigma, host.invsigma = train_model.mu, Symmetric(train_model.sigma), Symmetric(train_model.invsigma)
	host.beta, host.beta_old, host.topics = train_model.beta, copy(train_model.beta), train_model.topics
	dev = hipCTM(host)
	update_buffer!(dev)
	update_estep!(dev, niter, ntol, iter, tol)
	update_host!(dev)
	host.lambda, host.lambda_old, host.vsq, host.logzeta = dev.lambda, dev.lambda_old, dev.vsq, dev.logzeta
	return host
end

function topicdist(model::hipCTM, d::Integer)       # src/modelutils.jl:953-958
	(d <= length(model.corp)) || throw(CorpusError("document index outside corpus range."))
	return additive_logistic(model.lambda[d] + 0.5 * model.vsq[d])
end

# ---------------------------------------------------------------------------------------------- CTPF
# gpuCTPF replacement (src/gpuCTPF.jl:6-153).  train! ends with the recommendation tail of src/gpuCTPF.jl:711-731,
# which here is ONE call (device GEMM + segmented sorts) instead of M + U host sortperm calls.

mutable struct hipCTPF <: TopicModel
	K::Int; M::Int; V::Int; U::Int
	N::Vector{Int}; C::Vector{Int}; R::Vector{Int}
	corp::Corpus; topics::VectorList{Int}
	scores::Matrix{Float64}; libs::VectorList{Int}; drecs::VectorList{Int}; urecs::VectorList{Int}
	hyper::Vector{Float64}                                   # a, b, c, d, e, f, g, h  (src/CTPF.jl:81)
	alef::Matrix{Float64}; alef_old::Matrix{Float64}; he::Matrix{Float64}; he_old::Matrix{Float64}
	bet::Vector{Float64}; bet_old::Vector{Float64}; vav::Vector{Float64}; vav_old::Vector{Float64}
	dalet::Vector{Float64}; dalet_old::Vector{Float64}; het::Vector{Float64}; het_old::Vector{Float64}
	gimel::VectorList{Float64}; gimel_old::VectorList{Float64}; zayin::VectorList{Float64}; zayin_old::VectorList{Float64}
	elbo::Float64
	ctx::Ptr{Cvoid}; dcorp::Ptr{Cvoid}; handle::Ptr{Cvoid}
	comm::Union{hipComm, Nothing}
end

function hipCTPF(model::CTPF; device::Integer=0)
	ctx = tmvb_context(device)
	dcorp = tmvb_upload_corpus(ctx, model.corp)
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_ctpf_create, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), ctx, dcorp, model.K, h))
	m = hipCTPF(model.K, model.M, model.V, model.U, model.N, model.C, model.R, model.corp, model.topics, model.scores, model.libs,
		model.drecs, model.urecs, Float64[model.a, model.b, model.c, model.d, model.e, model.f, model.g, model.h],
		model.alef, model.alef_old, model.he, model.he_old, model.bet, model.bet_old, model.vav, model.vav_old,
		model.dalet, model.dalet_old, model.het, model.het_old, model.gimel, model.gimel_old, model.zayin, model.zayin_old,
		model.elbo, ctx, dcorp, h[], nothing)
	finalizer(m) do x
		ccall((:tmvb_ctpf_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), x.handle)
		tmvb_destroy_corpus(x.dcorp)
		tmvb_destroy_context(x.ctx)
	end
	return m
end

"update_buffer! (src/modelutils.jl:438-494), the *_old fields included (update_elbo! rebuilds phi / xi from them, src/CTPF.jl:239-240)."
function update_buffer!(model::hipCTPF)
	gim, zay = hcat(model.gimel...), hcat(model.zayin...)
	gim_old, zay_old = hcat(model.gimel_old...), hcat(model.zayin_old...)
	elbo = Ref{Float64}(model.elbo)
	GC.@preserve gim zay gim_old zay_old begin
		tmvb_check(ccall((:tmvb_ctpf_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
			model.handle, model.hyper, model.alef, model.he, model.bet, model.vav, model.dalet, model.het, gim, zay, elbo))
		tmvb_check(ccall((:tmvb_ctpf_set_state_old, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
			model.handle, model.alef_old, model.he_old, model.bet_old, model.vav_old, model.dalet_old, model.het_old, gim_old, zay_old))
	end
end

function update_host!(model::hipCTPF)       # src/modelutils.jl:539-570
	K, M, V, U = model.K, model.M, model.V, model.U
	alef = zeros(K, V); alef_old = zeros(K, V); he = zeros(K, U); he_old = zeros(K, U); rates = zeros(8K)
	gim = zeros(K, M); gim_old = zeros(K, M); zay = zeros(K, M); zay_old = zeros(K, M); elbo = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_ctpf_get_state, LIBTMVB), Cint,
		(Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
		model.handle, alef, alef_old, he, he_old, rates, gim, gim_old, zay, zay_old, elbo))
	model.alef, model.alef_old, model.he, model.he_old = alef, alef_old, he, he_old
	model.bet, model.vav, model.dalet, model.het = rates[1:K], rates[K+1:2K], rates[2K+1:3K], rates[3K+1:4K]
	model.bet_old, model.vav_old, model.dalet_old, model.het_old = rates[4K+1:5K], rates[5K+1:6K], rates[6K+1:7K], rates[7K+1:8K]
	model.gimel, model.gimel_old, model.zayin, model.zayin_old = cols(gim), cols(gim_old), cols(zay), cols(zay_old)
	model.elbo = elbo[]
end

# one Julia function per device operator (src/gpuCTPF.jl:314-670)
"update_xi! / update_phi! / update_zayin! / update_gimel! sweeps + update_he!(d) / update_alef!(d) of every document (src/CTPF.jl:353-365)."
update_estep!(model::hipCTPF, viter::Integer, vtol::Real) = tmvb_check(ccall((:tmvb_ctpf_estep, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), model.handle, viter, vtol))
"sum_d gimel_d, sum_d zayin_d (inputs of update_bet! / update_vav!)."
update_doc_sums!(model::hipCTPF) = tmvb_check(ccall((:tmvb_ctpf_reduce_docs, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
"update_he!, update_alef!, update_dalet!, update_het!, update_bet!, update_vav! in the reference's order (src/CTPF.jl:366-371)."
update_globals!(model::hipCTPF) = tmvb_check(ccall((:tmvb_ctpf_mstep, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
function update_elbo!(model::hipCTPF)
	e = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_ctpf_update_elbo, LIBTMVB), Cint, (Ptr{Cvoid}, Ref{Float64}), model.handle, e))
	model.elbo = e[]
end

function set_comm!(model::hipCTPF, comm::Union{hipComm, Nothing})
	tmvb_check(ccall((:tmvb_ctpf_set_comm, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), model.handle, comm === nothing ? C_NULL : comm.handle))
	model.comm = comm
	nothing
end

"scores / drecs / urecs of src/CTPF.jl:379-399 from the device-resident state (ids converted to 1-based)."
function update_recs!(model::hipCTPF)
	M, U = model.M, model.U
	scores = zeros(M, U); dr = zeros(Int32, U, M); dc = zeros(Int32, M); ur = zeros(Int32, M, U); uc = zeros(Int32, U)
	# the C arrays are row-major [M][U] / [U][M]: a column-major Julia (U, M) / (M, U) matrix has the same memory layout
	tmvb_check(ccall((:tmvb_ctpf_recommend, LIBTMVB), Cint,
		(Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Cfloat}, Ptr{Cfloat}),
		model.handle, scores, dr, dc, ur, uc, C_NULL, C_NULL))
	model.scores = scores
	model.drecs = [Int.(dr[1:dc[d], d]) .+ 1 for d in 1:M]
	model.urecs = [Int.(ur[1:uc[u], u]) .+ 1 for u in 1:U]
	nothing
end

"""
    train!(model::hipCTPF; iter=150, tol=1.0, viter=10, vtol=1/K^2, checkelbo=Inf, printelbo=true)

Signature of train!(::gpuCTPF) (src/gpuCTPF.jl:677-733), semantics of the CPU path (src/CTPF.jl:344-400).
"""
function train!(model::hipCTPF; iter::Integer=150, tol::Real=1.0, viter::Integer=10, vtol::Real=1/model.K^2, checkelbo::Real=Inf, printelbo::Bool=true)
	check_train_args([tol, vtol], [iter, viter], checkelbo)
	update_buffer!(model)
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(model.elbo)
	tmvb_check(ccall((:tmvb_ctpf_train, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		model.handle, iter, tol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	(iter > 0) && update_host!(model)
	Ebeta = model.alef ./ model.bet
	model.topics = hip_topics(model.ctx, Matrix{Float64}(Ebeta))                # reverse(sortperm(.)) per topic, src/CTPF.jl:376-377
	(model.comm === nothing) && update_recs!(model)                             # :379-399 (a shard ranks only its own documents)
	nothing
end

function topicdist(model::hipCTPF, d::Integer)      # src/modelutils.jl:960-965
	(d <= length(model.corp)) || throw(CorpusError("document index outside corpus range."))
	return model.gimel[d] / sum(model.gimel[d])
end

# ---------------------------------------------------------------------------------------------- fLDA / fCTM
# Filtered models (src/fLDA.jl, src/fCTM.jl).  The reference has no device types for them: `@gpu train!` on an fLDA / fCTM
# does nothing (src/macros.jl:274-278).  hipfLDA / hipfCTM follow the gpuLDA / gpuCTM pattern on the engine's filtered
# kernels.  tau / tau_old travel as flat vectors in corpus token order (vcat(model.tau...)).

splitdocs(flat::Vector{Float64}, N::Vector{Int}) = (o = cumsum([0; N]); [flat[o[d]+1:o[d+1]] for d in 1:length(N)])
flatdocs(v::VectorList{Float64}) = isempty(v) ? Float64[] : vcat(v...)

mutable struct hipfLDA <: TopicModel
	K::Int; M::Int; V::Int; N::Vector{Int}; C::Vector{Int}
	corp::Corpus; topics::VectorList{Int}
	eta::Float64; alpha::Vector{Float64}
	kappa::Vector{Float64}; kappa_old::Vector{Float64}
	beta::Matrix{Float64}; beta_old::Matrix{Float64}
	Elogtheta::VectorList{Float64}; Elogtheta_old::VectorList{Float64}; gamma::VectorList{Float64}
	tau::VectorList{Float64}; tau_old::VectorList{Float64}
	elbo::Float64
	ctx::Ptr{Cvoid}; dcorp::Ptr{Cvoid}; handle::Ptr{Cvoid}
	comm::Union{hipComm, Nothing}
end

function hipfLDA(model::fLDA; device::Integer=0)
	ctx = tmvb_context(device)
	dcorp = tmvb_upload_corpus(ctx, model.corp)
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_flda_create, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), ctx, dcorp, model.K, h))
	m = hipfLDA(model.K, model.M, model.V, model.N, model.C, model.corp, model.topics, model.eta, model.alpha, model.kappa, model.kappa_old,
		model.beta, model.beta_old, model.Elogtheta, model.Elogtheta_old, model.gamma, model.tau, model.tau_old, model.elbo, ctx, dcorp, h[], nothing)
	finalizer(m) do x
		ccall((:tmvb_flda_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), x.handle)
		tmvb_destroy_corpus(x.dcorp)
		tmvb_destroy_context(x.ctx)
	end
	return m
end

function update_buffer!(model::hipfLDA)
	beta, beta_old = Matrix{Float64}(model.beta), Matrix{Float64}(model.beta_old)
	gamma, El, Elo = hcat(model.gamma...), hcat(model.Elogtheta...), hcat(model.Elogtheta_old...)
	tau, tau_old = flatdocs(model.tau), flatdocs(model.tau_old)
	eta = Ref{Float64}(model.eta); elbo = Ref{Float64}(model.elbo)
	GC.@preserve beta beta_old gamma El Elo tau tau_old begin
		tmvb_check(ccall((:tmvb_flda_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
			model.handle, eta, model.alpha, model.kappa, model.kappa_old, beta, beta_old, gamma, El, Elo, tau, tau_old, elbo))
	end
end

function update_host!(model::hipfLDA)
	K, M, V, nnz = model.K, model.M, model.V, sum(model.N)
	alpha = zeros(K); kappa = zeros(V); kappa_old = zeros(V); beta = zeros(K, V); beta_old = zeros(K, V)
	gamma = zeros(K, M); El = zeros(K, M); Elo = zeros(K, M); tau = zeros(nnz); tau_old = zeros(nnz)
	eta = Ref{Float64}(0.0); elbo = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_flda_get_state, LIBTMVB), Cint,
		(Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
		model.handle, eta, alpha, kappa, kappa_old, beta, beta_old, gamma, El, Elo, tau, tau_old, elbo))
	model.eta, model.alpha, model.kappa, model.kappa_old, model.beta, model.beta_old = eta[], alpha, kappa, kappa_old, beta, beta_old
	model.gamma, model.Elogtheta, model.Elogtheta_old = cols(gamma), cols(El), cols(Elo)
	model.tau, model.tau_old = splitdocs(tau, model.N), splitdocs(tau_old, model.N)
	model.elbo = elbo[]
end

"update_phi! / update_tau! / update_gamma! / update_Elogtheta! sweeps + update_beta!(model, d) + update_kappa!(model, d) (src/fLDA.jl:222-236)."
update_estep!(model::hipfLDA, viter::Integer, vtol::Real) = tmvb_check(ccall((:tmvb_flda_estep, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), model.handle, viter, vtol))
update_Elogtheta_sum!(model::hipfLDA) = tmvb_check(ccall((:tmvb_flda_reduce_docs, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
"update_beta! and update_kappa! (src/fLDA.jl:152, :138)."
update_beta!(model::hipfLDA) = tmvb_check(ccall((:tmvb_flda_update_beta, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
update_alpha!(model::hipfLDA, niter::Integer, ntol::Real) = tmvb_check(ccall((:tmvb_flda_update_alpha, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64), model.handle, niter, ntol))
update_eta!(model::hipfLDA) = tmvb_check(ccall((:tmvb_flda_update_eta, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))      # src/fLDA.jl:122
function update_elbo!(model::hipfLDA)
	e = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_flda_update_elbo, LIBTMVB), Cint, (Ptr{Cvoid}, Ref{Float64}), model.handle, e))
	model.elbo = e[]
end

"Document shard of a corpus of M_total documents and C_total tokens (sum of all counts; eta's denominator, src/fLDA.jl:123)."
function set_comm!(model::hipfLDA, comm::Union{hipComm, Nothing}, M_total::Integer, C_total::Integer)
	tmvb_check(ccall((:tmvb_flda_set_comm, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64), model.handle, comm === nothing ? C_NULL : comm.handle, M_total, C_total))
	model.comm = comm
	nothing
end

"train!(model::fLDA; ...) (src/fLDA.jl:213-247) on the device."
function train!(model::hipfLDA; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/model.K^2, viter::Integer=10, vtol::Real=1/model.K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	update_buffer!(model)
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(model.elbo)
	tmvb_check(ccall((:tmvb_flda_train, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		model.handle, iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	(iter > 0) && update_host!(model)
	model.topics = hip_topics(model.ctx, model.beta)                             # reverse(sortperm(.)) per topic
	nothing
end

function train!(models::Vector{hipfLDA}; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/models[1].K^2, viter::Integer=10, vtol::Real=1/models[1].K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	foreach(update_buffer!, models)
	hs = Ptr{Cvoid}[m.handle for m in models]
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(models[1].elbo)
	tmvb_check(ccall((:tmvb_flda_train_group, LIBTMVB), Cint,
		(Ptr{Ptr{Cvoid}}, Int32, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		hs, length(hs), iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	for m in models
		(iter > 0) && update_host!(m)
		m.topics = hip_topics(m.ctx, m.beta)
	end
	nothing
end

"""
predict (src/modelutils.jl:857-883) on the device.  As in the reference only alpha, beta and topics come from the trained model
(:866-868): kappa and eta are those of the fresh fLDA(corp, K).  The reference's loop tests `vtol`, which that function never
defines (:877); `tol` is used here.
"""
function predict(corp::Corpus, train_model::hipfLDA; iter::Integer=10, tol::Real=1/train_model.K^2)
	check_corp(corp)
	(corp.vocab == train_model.corp.vocab)	|| throw(CorpusError("predict corpus and train_model corpus must have identical vocabularies."))
	(tol >= 0)								|| throw(ArgumentError("tolerance parameter must be nonnegative."))
	(iter >= 0)								|| throw(ArgumentError("iteration parameter must be nonnegative."))
	host = fLDA(corp, train_model.K)
	host.alpha, host.beta, host.beta_old, host.topics = train_model.alpha, train_model.beta, copy(train_model.beta), train_model.topics
	dev = hipfLDA(host)
	update_buffer!(dev)
	update_estep!(dev, iter, tol)
	update_host!(dev)
	host.gamma, host.Elogtheta, host.Elogtheta_old, host.tau, host.tau_old = dev.gamma, dev.Elogtheta, dev.Elogtheta_old, dev.tau, dev.tau_old
	return host
end

function topicdist(model::hipfLDA, d::Integer)      # src/modelutils.jl:946-951
	(d <= length(model.corp)) || throw(CorpusError("document index outside corpus range."))
	return model.gamma[d] / sum(model.gamma[d])
end

mutable struct hipfCTM <: TopicModel
	K::Int; M::Int; V::Int; N::Vector{Int}; C::Vector{Int}
	corp::Corpus; topics::VectorList{Int}
	eta::Float64
	mu::Vector{Float64}; sigma::Matrix{Float64}; invsigma::Matrix{Float64}
	kappa::Vector{Float64}; kappa_old::Vector{Float64}
	beta::Matrix{Float64}; beta_old::Matrix{Float64}
	lambda::VectorList{Float64}; lambda_old::VectorList{Float64}; vsq::VectorList{Float64}; logzeta::Vector{Float64}
	tau::VectorList{Float64}; tau_old::VectorList{Float64}
	elbo::Float64
	ctx::Ptr{Cvoid}; dcorp::Ptr{Cvoid}; handle::Ptr{Cvoid}
	comm::Union{hipComm, Nothing}
end

function hipfCTM(model::fCTM; device::Integer=0)
	ctx = tmvb_context(device)
	dcorp = tmvb_upload_corpus(ctx, model.corp)
	h = Ref{Ptr{Cvoid}}(C_NULL)
	tmvb_check(ccall((:tmvb_fctm_create, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ref{Ptr{Cvoid}}), ctx, dcorp, model.K, h))
	m = hipfCTM(model.K, model.M, model.V, model.N, model.C, model.corp, model.topics, model.eta, model.mu, Matrix(model.sigma),
		Matrix(model.invsigma), model.kappa, model.kappa_old, model.beta, model.beta_old, model.lambda, model.lambda_old, model.vsq,
		model.logzeta, model.tau, model.tau_old, model.elbo, ctx, dcorp, h[], nothing)
	finalizer(m) do x
		ccall((:tmvb_fctm_destroy, LIBTMVB), Cint, (Ptr{Cvoid},), x.handle)
		tmvb_destroy_corpus(x.dcorp)
		tmvb_destroy_context(x.ctx)
	end
	return m
end

function update_buffer!(model::hipfCTM)
	beta, beta_old = Matrix{Float64}(model.beta), Matrix{Float64}(model.beta_old)
	lam, lam_old, vsq = hcat(model.lambda...), hcat(model.lambda_old...), hcat(model.vsq...)
	tau, tau_old = flatdocs(model.tau), flatdocs(model.tau_old)
	eta = Ref{Float64}(model.eta); elbo = Ref{Float64}(model.elbo)
	GC.@preserve beta beta_old lam lam_old vsq tau tau_old begin
		tmvb_check(ccall((:tmvb_fctm_set_state, LIBTMVB), Cint,
			(Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
			model.handle, eta, model.mu, model.sigma, model.invsigma, model.kappa, model.kappa_old, beta, beta_old, lam, lam_old, vsq, model.logzeta, tau, tau_old, elbo))
	end
end

function update_host!(model::hipfCTM)
	K, M, V, nnz = model.K, model.M, model.V, sum(model.N)
	mu = zeros(K); sg = zeros(K, K); isg = zeros(K, K); kappa = zeros(V); kappa_old = zeros(V); beta = zeros(K, V); beta_old = zeros(K, V)
	lam = zeros(K, M); lam_old = zeros(K, M); vsq = zeros(K, M); lz = zeros(M); tau = zeros(nnz); tau_old = zeros(nnz)
	eta = Ref{Float64}(0.0); elbo = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_fctm_get_state, LIBTMVB), Cint,
		(Ptr{Cvoid}, Ref{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Float64}),
		model.handle, eta, mu, sg, isg, kappa, kappa_old, beta, beta_old, lam, lam_old, vsq, lz, tau, tau_old, elbo))
	model.eta, model.mu, model.sigma, model.invsigma = eta[], mu, sg, isg
	model.kappa, model.kappa_old, model.beta, model.beta_old = kappa, kappa_old, beta, beta_old
	model.lambda, model.lambda_old, model.vsq, model.logzeta = cols(lam), cols(lam_old), cols(vsq), lz
	model.tau, model.tau_old = splitdocs(tau, model.N), splitdocs(tau_old, model.N)
	model.elbo = elbo[]
end

"update_phi! / update_tau! / update_logzeta! / update_lambda! / update_vsq! sweeps + update_beta!(model, d) + update_kappa!(model, d) (src/fCTM.jl:233-248)."
update_estep!(model::hipfCTM, niter::Integer, ntol::Real, viter::Integer, vtol::Real) = tmvb_check(ccall((:tmvb_fctm_estep, LIBTMVB), Cint, (Ptr{Cvoid}, Int32, Float64, Int32, Float64), model.handle, niter, ntol, viter, vtol))
update_doc_sums!(model::hipfCTM) = tmvb_check(ccall((:tmvb_fctm_reduce_docs, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
"update_beta! and update_kappa! (src/fCTM.jl:148, :134)."
update_beta!(model::hipfCTM) = tmvb_check(ccall((:tmvb_fctm_update_beta, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))
update_sigma!(model::hipfCTM) = tmvb_check(ccall((:tmvb_fctm_update_sigma, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))  # src/fCTM.jl:128 -- before update_mu!
update_mu!(model::hipfCTM) = tmvb_check(ccall((:tmvb_fctm_update_mu, LIBTMVB), Cint, (Ptr{Cvoid},), model.handle))        # :122
function update_elbo!(model::hipfCTM)
	e = Ref{Float64}(0.0)
	tmvb_check(ccall((:tmvb_fctm_update_elbo, LIBTMVB), Cint, (Ptr{Cvoid}, Ref{Float64}), model.handle, e))
	model.elbo = e[]
end

function set_comm!(model::hipfCTM, comm::Union{hipComm, Nothing}, M_total::Integer)
	tmvb_check(ccall((:tmvb_fctm_set_comm, LIBTMVB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), model.handle, comm === nothing ? C_NULL : comm.handle, M_total))
	model.comm = comm
	nothing
end

"train!(model::fCTM; ...) (src/fCTM.jl:226-262) on the device; eta stays fixed (update_eta! is commented out, :253)."
function train!(model::hipfCTM; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/model.K^2, viter::Integer=10, vtol::Real=1/model.K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	update_buffer!(model)
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(model.elbo)
	tmvb_check(ccall((:tmvb_fctm_train, LIBTMVB), Cint,
		(Ptr{Cvoid}, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		model.handle, iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	(iter > 0) && update_host!(model)
	model.topics = hip_topics(model.ctx, model.beta)                             # reverse(sortperm(.)) per topic
	nothing
end

function train!(models::Vector{hipfCTM}; iter::Integer=150, tol::Real=1.0, niter::Integer=1000, ntol::Real=1/models[1].K^2, viter::Integer=10, vtol::Real=1/models[1].K^2, checkelbo::Real=1, printelbo::Bool=true)
	check_train_args([tol, ntol, vtol], [iter, niter, viter], checkelbo)
	foreach(update_buffer!, models)
	hs = Ptr{Cvoid}[m.handle for m in models]
	traj = fill(NaN, max(iter, 1)); done = Ref{Int32}(0); base = Ref{Float64}(models[1].elbo)
	tmvb_check(ccall((:tmvb_fctm_train_group, LIBTMVB), Cint,
		(Ptr{Ptr{Cvoid}}, Int32, Int32, Float64, Int32, Float64, Int32, Float64, Int32, Ptr{Float64}, Ref{Int32}, Ref{Float64}),
		hs, length(hs), iter, tol, niter, ntol, viter, vtol, checkelbo_arg(checkelbo), traj, done, base))
	printelbo && print_delbo(traj, done[], base[])
	for m in models
		(iter > 0) && update_host!(m)
		m.topics = hip_topics(m.ctx, m.beta)
	end
	nothing
end

"predict (src/modelutils.jl:915-943) on the device; mu / sigma / invsigma / beta / topics from the trained model (:924-928), `tol` for the reference's undefined `vtol` (:937)."
function predict(corp::Corpus, train_model::hipfCTM; iter::Integer=10, tol::Real=1/train_model.K^2, niter::Integer=1000, ntol::Real=1/train_model.K^2)
	check_corp(corp)
	(corp.vocab == train_model.corp.vocab)	|| throw(CorpusError("predict corpus and train_model corpus must have identical vocabularies."))
	all([tol, ntol] .>= 0)					|| throw(ArgumentError("tolerance parameters must be nonnegative."))
	all([iter, niter] .>= 0)				|| throw(ArgumentError("iteration parameters must be nonnegative."))
	host = fCTM(corp, train_model.K)
	host.mu, host.sigma, host.invsigma = train_model.mu, Symmetric(train_model.sigma), Symmetric(train_model.invsigma)
	host.beta, host.beta_old, host.topics = train_model.beta, copy(train_model.beta), train_model.topics
	dev = hipfCTM(host)
	update_buffer!(dev)
	update_estep!(dev, niter, ntol, iter, tol)
	update_host!(dev)
	host.lambda, host.lambda_old, host.vsq, host.logzeta, host.tau, host.tau_old = dev.lambda, dev.lambda_old, dev.vsq, dev.logzeta, dev.tau, dev.tau_old
	return host
end

function topicdist(model::hipfCTM, d::Integer)      # src/modelutils.jl:953-958
	(d <= length(model.corp)) || throw(CorpusError("document index outside corpus range."))
	return additive_logistic(model.lambda[d] + 0.5 * model.vsq[d])
end

# ---------------------------------------------------------------------------------------------- gendoc / gencorp
# gendoc / gencorp (src/modelutils.jl:594-649) on the device (tmvb_lda_gencorp / tmvb_ctm_gencorp): Poisson lengths, Dirichlet or
# logistic-normal theta, two categorical draws per token, condensed on the device.  Methods for the hip types only, like predict's: the
# package's own gendoc / gencorp keep serving the host models (its CTM method throws at :626; `gencorp(hipCTM(model), M)` is the way round).
# The reference draws from Julia's global RNG;
# here `seed` names the corpus (same seed, same documents; documents d0+1 .. d0+m of a corpus are `doc_offset=d0, M=m`).  Terms of a document
# come out sorted ascending.

"tmvb_gencorp_t (include/tmvb.h), field for field."
mutable struct TmvbGencorp
	M::Int64; nnz::Int64; sum_counts::Int64
	doc_ptr::Ptr{Int64}; terms::Ptr{Int32}; counts::Ptr{Int32}
	log_theta::Ptr{Float32}; doc_topic::Ptr{Int32}; topic_term::Ptr{Int64}
	ms_tables::Float32; ms_docs::Float32; ms_tokens::Float32; ms_condense::Float32
	TmvbGencorp() = new(0, 0, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 0f0, 0f0, 0f0, 0f0)
end

const DirichletModels = Union{hipLDA, hipfLDA}
const LogisticNormalModels = Union{hipCTM, hipfCTM}

function gencorp_docs(out::TmvbGencorp)
	doc_ptr = unsafe_wrap(Array, out.doc_ptr, out.M + 1)
	terms = unsafe_wrap(Array, out.terms, out.nnz); counts = unsafe_wrap(Array, out.counts, out.nnz)
	[Document(terms=Int.(terms[doc_ptr[d]+1:doc_ptr[d+1]]) .+ 1, counts=Int.(counts[doc_ptr[d]+1:doc_ptr[d+1]])) for d in 1:out.M]
end

function hip_gencorp(model::DirichletModels, M::Integer, laplace_smooth::Real, seed::Integer, doc_offset::Integer)
	ctx = model.ctx
	out = TmvbGencorp()
	alpha = Vector{Float64}(model.alpha); beta = Matrix{Float64}(model.beta)
	GC.@preserve out alpha beta begin
		tmvb_check(ccall((:tmvb_lda_gencorp, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Float64, Int64, Int32, Ptr{Cvoid}),
			ctx, model.K, model.V, alpha, beta, M, doc_offset, mean(model.C), laplace_smooth, seed, 0, pointer_from_objref(out)))
		docs = gencorp_docs(out)
		ccall((:tmvb_gencorp_free, LIBTMVB), Cvoid, (Ptr{Cvoid},), pointer_from_objref(out))
		return docs
	end
end

function hip_gencorp(model::LogisticNormalModels, M::Integer, laplace_smooth::Real, seed::Integer, doc_offset::Integer)
	ctx = model.ctx
	out = TmvbGencorp()
	mu = Vector{Float64}(model.mu); sigma = Matrix{Float64}(model.sigma); beta = Matrix{Float64}(model.beta)
	GC.@preserve out mu sigma beta begin
		tmvb_check(ccall((:tmvb_ctm_gencorp, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Int64, Int64, Float64, Float64, Int64, Int32, Ptr{Cvoid}),
			ctx, model.K, model.V, mu, sigma, beta, M, doc_offset, mean(model.C), laplace_smooth, seed, 0, pointer_from_objref(out)))
		docs = gencorp_docs(out)
		ccall((:tmvb_gencorp_free, LIBTMVB), Cvoid, (Ptr{Cvoid},), pointer_from_objref(out))
		return docs
	end
end

"gendoc (src/modelutils.jl:594-633) on the device: document 1 of the corpus `seed` names."
function gendoc(model::Union{DirichletModels, LogisticNormalModels}, laplace_smooth::Real=0.0; seed::Integer=rand(Int64))
	(laplace_smooth >= 0) || throw(ArgumentError("laplace_smooth parameter must be nonnegative."))
	return hip_gencorp(model, 1, laplace_smooth, seed, 0)[1]
end

"gencorp (src/modelutils.jl:642-649) on the device."
function gencorp(model::Union{DirichletModels, LogisticNormalModels}, M::Integer; laplace_smooth::Real=0.0, seed::Integer=rand(Int64), doc_offset::Integer=0)
	(M > 0)					|| throw(ArgumentError("corp_size parameter must be a positive integer."))
	(laplace_smooth >= 0)	|| throw(ArgumentError("laplace_smooth parameter must be nonnegative."))
	corp = Corpus(vocab=model.corp.vocab, users=model.corp.users)
	corp.docs = hip_gencorp(model, M, laplace_smooth, seed, doc_offset)
	return corp
end

# ---------------------------------------------------------------------------------------------- held-out evaluation
# Document-completion perplexity (the reference has no such function; SURVEY section 8(f) item 1 names it as the purpose of predict):
# split_corp holds every token occurrence of a corpus out with probability frac (tmvb_corpus_split: a pure function of seed, document and
# occurrence, Philox4x32-10 -- the same seed gives the same split, doc_offset reproduces a slice), heldout_loglik folds the observed side in
# with the hip model's predict, takes topicdist of every document as theta and scores the held-out side under model.beta on the device
# (tmvb_heldout_loglik).  The filtered models' kappa / tau take no part in the score, as in the reference's gendoc.

"tmvb_split_t (include/tmvb.h), field for field."
mutable struct TmvbSplit
	M::Int64; nnz_obs::Int64; nnz_held::Int64; sum_obs::Int64; sum_held::Int64
	obs_ptr::Ptr{Int64}; obs_terms::Ptr{Int32}; obs_counts::Ptr{Int32}
	held_ptr::Ptr{Int64}; held_terms::Ptr{Int32}; held_counts::Ptr{Int32}
	ms_draw::Float32; ms_compact::Float32
	TmvbSplit() = new(0, 0, 0, 0, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, 0f0, 0f0)
end

function corp_csr(corp::Corpus)
	doc_ptr = Int64[0; cumsum([length(doc.terms) for doc in corp])]
	terms   = Int32.(reduce(vcat, [doc.terms for doc in corp]; init=Int[]) .- 1)
	counts  = Int32.(reduce(vcat, [doc.counts for doc in corp]; init=Int[]))
	return doc_ptr, terms, counts
end

function split_docs(p::Ptr{Int64}, t::Ptr{Int32}, c::Ptr{Int32}, M::Integer, nnz::Integer)
	doc_ptr = unsafe_wrap(Array, p, M + 1)
	terms = unsafe_wrap(Array, t, nnz); counts = unsafe_wrap(Array, c, nnz)
	[Document(terms=Int.(terms[doc_ptr[d]+1:doc_ptr[d+1]]) .+ 1, counts=Int.(counts[doc_ptr[d]+1:doc_ptr[d+1]])) for d in 1:M]
end

"(observed, heldout): two corpora over the vocabulary of `corp`; every token occurrence is held out with probability frac."
function split_corp(corp::Corpus; frac::Real=0.5, seed::Integer=0, doc_offset::Integer=0, device::Integer=0)
	check_corp(corp)
	M, V, U = size(corp)
	doc_ptr, terms, counts = corp_csr(corp)
	ctx = tmvb_context(device)
	out = TmvbSplit()
	GC.@preserve out doc_ptr terms counts begin
		rc = ccall((:tmvb_corpus_split, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Float64, Int64, Int64, Ptr{Cvoid}),
			ctx, M, V, doc_ptr, terms, counts, frac, seed, doc_offset, pointer_from_objref(out))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
		observed = Corpus(vocab=corp.vocab, users=corp.users); heldout = Corpus(vocab=corp.vocab, users=corp.users)
		observed.docs = split_docs(out.obs_ptr, out.obs_terms, out.obs_counts, out.M, out.nnz_obs)
		heldout.docs = split_docs(out.held_ptr, out.held_terms, out.held_counts, out.M, out.nnz_held)
		ccall((:tmvb_split_free, LIBTMVB), Cvoid, (Ptr{Cvoid},), pointer_from_objref(out))
		return observed, heldout
	end
end

"""
(ll, tokens, zero_prob_tokens, perplexity) of the held-out words: ll[d] = sum_n c_n log(sum_k theta[k,d] beta'[k,w_n]) with theta the
topicdist of predict(observed, model) and beta' = (beta + laplace_smooth) / (1 + laplace_smooth V); perplexity = exp(-sum(ll) / sum(tokens)).
"""
function heldout_loglik(model::Union{DirichletModels, LogisticNormalModels}, observed::Corpus, heldout::Corpus; laplace_smooth::Real=0.0, kwargs...)
	(heldout.vocab == model.corp.vocab)		|| throw(CorpusError("predict corpus and train_model corpus must have identical vocabularies."))
	(length(observed) == length(heldout))	|| throw(CorpusError("observed and heldout corpora must hold the same documents."))
	(laplace_smooth >= 0)					|| throw(ArgumentError("laplace_smooth parameter must be nonnegative."))
	pred = predict(observed, model; kwargs...)
	M = length(heldout)
	theta = Matrix{Float64}(undef, model.K, M)
	for d in 1:M
		theta[:,d] = topicdist(pred, d)
	end
	beta = Matrix{Float64}(model.beta)
	doc_ptr, terms, counts = corp_csr(heldout)
	ll = zeros(Float64, M); tokens = zeros(Int64, M); zero_prob = Ref{Int64}(0); ms = Ref{Float32}(0f0)
	GC.@preserve theta beta doc_ptr terms counts ll tokens begin
		tmvb_check(ccall((:tmvb_heldout_loglik, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Float64, Ptr{Float64}, Ptr{Int64}, Ref{Int64}, Ref{Float32}),
			model.ctx, model.K, model.V, M, theta, beta, doc_ptr, terms, counts, laplace_smooth, ll, tokens, zero_prob, ms))
	end
	n = sum(tokens)
	ppl = n == 0 ? NaN : (any(isinf, ll) ? Inf : exp(-sum(ll) / n))
	return (ll=ll, tokens=tokens, zero_prob_tokens=zero_prob[], perplexity=ppl)
end

"Document-completion perplexity of `corp` (unseen documents) under `model`: split_corp, then heldout_loglik."
function perplexity(model::Union{DirichletModels, LogisticNormalModels}, corp::Corpus; frac::Real=0.5, seed::Integer=0, kwargs...)
	observed, heldout = split_corp(corp; frac=frac, seed=seed)
	return heldout_loglik(model, observed, heldout; kwargs...).perplexity
end

# ---------------------------------------------------------------------------------------------- topic coherence
# Whether the top words of a topic occur together in documents (the reference has no such function): tmvb_corpus_codocfreq counts, for
# every topic, the documents of `corp` that contain both words of every pair of its topn top words (a bit matrix over the corpus on the
# device, AND / popcount over pairs; exact integers, additive over document shards), tmvb_coherence_from_counts turns the counts into UMass
# (Mimno et al. 2011, as a mean over the defined pairs) and NPMI with the document as the window (Lau et al. 2014) on the host.

"tmvb_codf_info_t (include/tmvb.h), field for field."
mutable struct TmvbCodfInfo
	n_slots::Int64; n_batches::Int32
	ms_bitset::Float32; ms_pairs::Float32
	TmvbCodfInfo() = new(0, 0, 0f0, 0f0)
end

"""
(codf, df, umass, npmi, undefined_pairs, diversity) of the first `topn` words of every topic of `model` against `corp`:
codf[i,j,k] = documents that contain both the i-th and the j-th top word of topic k, df[i,k] its diagonal; umass[k] is NaN where no pair is
defined; diversity = distinct top words / (K topn).
"""
function coherence(model::TopicModel, corp::Corpus; topn::Integer=10, device::Integer=0, max_bitset_bytes::Integer=0)
	(2 <= topn <= 64)					|| throw(ArgumentError("topn must be an integer in [2, 64]."))
	M, V, U = size(corp)
	(V == model.V)						|| throw(CorpusError("coherence corpus and model must have identical vocabularies."))
	(topn <= V)							|| throw(ArgumentError("topn = $topn above the vocabulary size."))
	K = model.K
	top = Matrix{Int32}(undef, topn, K)									# column k = row k of the C array top[K][N]
	for k in 1:K
		top[:,k] = Int32.(model.topics[k][1:topn] .- 1)
	end
	doc_ptr, terms, counts = corp_csr(corp)
	codf = zeros(Int64, topn, topn, K)									# column-major (j, i, k) = C's codf[k][i][j]; symmetric in (i, j)
	info = TmvbCodfInfo()
	ctx = tmvb_context(device)
	GC.@preserve info doc_ptr terms counts top codf begin
		rc = ccall((:tmvb_corpus_codocfreq, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Cvoid}),
			ctx, M, V, doc_ptr, terms, counts, K, topn, top, max_bitset_bytes, codf, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	umass = zeros(Float64, K); npmi = zeros(Float64, K); undefined_pairs = zeros(Int32, K)
	GC.@preserve codf umass npmi undefined_pairs begin
		tmvb_check(ccall((:tmvb_coherence_from_counts, LIBTMVB), Cint,
			(Int32, Int32, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}),
			K, topn, M, codf, umass, npmi, undefined_pairs))
	end
	df = [codf[i,i,k] for i in 1:topn, k in 1:K]
	return (codf=codf, df=df, umass=umass, npmi=npmi, undefined_pairs=Int.(undefined_pairs),
			diversity=length(unique(top)) / (K * topn), ms=(bitset=info.ms_bitset, pairs=info.ms_pairs))
end

# ---------------------------------------------------------------------------------------------- nearest documents in topic space
# Which documents are about the same things as this one (the reference stops at topicdist(model, d)): tmvb_topic_neighbors scores every query
# against every document of the model on the device (fp32 features, the f32 MFMA = the ascending fmaf chain) and keeps, per query, the topn
# best under the total order (score descending, index ascending); the score matrix never exists.

"tmvb_neighbors_info_t (include/tmvb.h), field for field."
mutable struct TmvbNeighborsInfo
	splits::Int32; kp::Int32
	ms_prep::Float32; ms_scan::Float32; ms_merge::Float32
	TmvbNeighborsInfo() = new(0, 0, 0f0, 0f0, 0f0)
end

"K x M topic proportions: column d is topicdist(model, d)."
topic_proportions(model::DirichletModels) = hcat([g / sum(g) for g in model.gamma]...)
topic_proportions(model::LogisticNormalModels) = hcat([additive_logistic(model.lambda[d] + 0.5 * model.vsq[d]) for d in 1:length(model.lambda)]...)
topic_proportions(model::hipCTPF) = hcat([g / sum(g) for g in model.gimel]...)

const NB_METRICS = Dict(:dot => 0, :hellinger => 1, :cosine => 2)

"""
(idx, score, distance, count) of the `topn` documents of `model` nearest to each document of `docs` (1-based like topicdist; a contiguous
range, by default every document), the document itself excluded -- or, with `queries` (another model over other documents, what predict
returned), nearest to each of ITS documents, nothing excluded.  idx[j, q] is 1-based, 0 past count[q]; metric = :hellinger (score =
Bhattacharyya coefficient, distance = sqrt(max(0, 1 - score))), :cosine (distance = 1 - score) or :dot (distance = nothing).
"""
function docsim(model::TopicModel; docs::AbstractUnitRange{<:Integer}=1:0, topn::Integer=10, metric::Symbol=:hellinger, queries=nothing, device::Integer=0)
	haskey(NB_METRICS, metric)			|| throw(ArgumentError("metric must be :dot, :hellinger or :cosine."))
	(1 <= topn <= 64)					|| throw(ArgumentError("topn must be an integer in [1, 64]."))
	xd = Matrix{Float64}(topic_proportions(model))
	K, Md = size(xd)
	src = queries === nothing ? xd : Matrix{Float64}(topic_proportions(queries))
	(size(src, 1) == K)					|| throw(TopicModelError("queries and model must have the same number of topics."))
	docs = isempty(docs) ? (1:size(src, 2)) : docs
	(1 <= first(docs) && last(docs) <= size(src, 2))	|| throw(CorpusError("document index outside corpus range."))
	Mq = length(docs)
	xq = queries === nothing ? xd : src[:, docs]						# explicit query rows only with `queries`
	idx = zeros(Int32, topn, Mq); score = zeros(Float32, topn, Mq); count = zeros(Int32, Mq)	# column-major (j, q) = C's [q][j]
	info = TmvbNeighborsInfo()
	ctx = tmvb_context(device)
	GC.@preserve info xd xq idx score count begin
		rc = ccall((:tmvb_topic_neighbors, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
			ctx, K, NB_METRICS[metric], Md, xd, Mq, queries === nothing ? Ptr{Float64}(C_NULL) : pointer(xq), queries === nothing ? first(docs) - 1 : 0,
			topn, 0, idx, score, count, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	s = Float64.(score)
	distance = metric == :hellinger ? sqrt.(max.(0.0, 1.0 .- s)) : metric == :cosine ? 1.0 .- s : nothing
	return (idx=Int.(idx) .+ 1, score=score, distance=distance, count=Int.(count),
			ms=(prep=info.ms_prep, scan=info.ms_scan, merge=info.ms_merge), splits=Int(info.splits))
end

# ---------------------------------------------------------------------------------------------- cluster documents in topic space
# Which documents belong together: tmvb_topic_kmeans runs Lloyd's k-means on the topic proportions on the device -- fp32 features, the assignment
# on the f32 MFMA with the arg-max in its epilogue, fixed-order fp64 sums for the centroids and the inertia, k-means++ seeding.

"tmvb_kmeans_info_t (include/tmvb.h), field for field."
mutable struct TmvbKMeansInfo
	iters::Int32; stop::Int32; n_empty::Int32; kp::Int32
	moved_last::Int64
	ms_prep::Float32; ms_seed::Float32; ms_assign::Float32; ms_update::Float32
	TmvbKMeansInfo() = new(0, 0, 0, 0, 0, 0f0, 0f0, 0f0, 0f0)
end

const KM_METRICS = Dict(:euclid => 0, :hellinger => 1, :cosine => 2)

"""
k-means of the documents of `model` in topic space into `k` clusters (on `theta`, K x M topic proportions, if given: e.g. those of what predict
returned).  labels[d] is 1-based; centroids is K x k in feature space (sqrt of proportions for :hellinger, unit vectors for :cosine), profiles
the centroids as topic proportions; init = nothing seeds with k-means++ (`seed`), a K x k matrix starts from those centroids; maxiter = 0
only assigns.  stop: 0 maxiter, 1 no label moved, 2 tol.  seeds are 1-based document ids, 0 when the centroids were given.
"""
function kmeans(model::TopicModel, k::Integer; metric::Symbol=:hellinger, init=nothing, seed::Integer=0, maxiter::Integer=100, tol::Real=0.0,
				theta=nothing, device::Integer=0)
	haskey(KM_METRICS, metric)			|| throw(ArgumentError("metric must be :euclid, :hellinger or :cosine."))
	x = Matrix{Float64}(theta === nothing ? topic_proportions(model) : theta)
	K, M = size(x)
	(1 <= k <= min(M, 1024))			|| throw(ArgumentError("k must be an integer in [1, min(M, 1024)]."))
	(0 <= maxiter <= 10000)				|| throw(ArgumentError("maxiter must be an integer in [0, 10000]."))
	c0 = init === nothing ? zeros(Float64, 0, 0) : Matrix{Float64}(init)
	(init === nothing || size(c0) == (K, k))	|| throw(TopicModelError("init must be a K x k matrix of centroids."))
	label = zeros(Int32, M); centroid = zeros(Float64, K, k); count = zeros(Int64, k); dist2 = zeros(Float32, M)
	inertia = fill(NaN, maxiter + 1); seeds = zeros(Int32, k)
	info = TmvbKMeansInfo()
	ctx = tmvb_context(device)
	GC.@preserve info x c0 label centroid count dist2 inertia seeds begin
		rc = ccall((:tmvb_topic_kmeans, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Float64}, Int32, Ptr{Float64}, Int64, Int32, Float64, Ptr{Int32}, Ptr{Float64}, Ptr{Int64}, Ptr{Float32},
			 Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}),
			ctx, K, KM_METRICS[metric], M, x, k, init === nothing ? Ptr{Float64}(C_NULL) : pointer(c0), seed, maxiter, tol, label, centroid, count, dist2,
			inertia, seeds, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	c = metric == :hellinger ? centroid .^ 2 : centroid
	d = Float64.(dist2)
	distance = metric == :hellinger ? sqrt.(0.5 .* d) : metric == :euclid ? sqrt.(d) : 0.5 .* d
	return (labels=Int.(label) .+ 1, centroids=centroid, profiles=c ./ sum(c, dims=1), counts=Int.(count), dist2=dist2, distance=distance,
			inertia=inertia[1:info.iters + 1], iters=Int(info.iters), stop=Int(info.stop), n_empty=Int(info.n_empty), seeds=Int.(seeds) .+ 1,
			ms=(prep=info.ms_prep, seed=info.ms_seed, assign=info.ms_assign, update=info.ms_update))
end

# ---------------------------------------------------------------------------------------------- map documents in two dimensions
# Where the documents lie: tmvb_map_affinity turns the neighbour lists of tmvb_topic_neighbors into t-SNE's input similarities (entropy search in
# fp64 on a fixed schedule, symmetrised CSR), tmvb_map_layout runs the gradient descent with the repulsive term over ALL pairs in a fixed order --
# no Barnes-Hut tree, no FFT grid --, so equal inputs give equal bytes.

"tmvb_map_params_t (include/tmvb.h), field for field."
mutable struct TmvbMapParams
	iters::Int32; iter0::Int32; exag_iters::Int32; check::Int32; j_split::Int32; reserved::Int32
	seed::Int64
	exaggeration::Float64; min_grad_norm::Float64
	momentum0::Float32; momentum1::Float32; eta::Float32; min_gain::Float32
end

"tmvb_map_info_t (include/tmvb.h), field for field."
mutable struct TmvbMapInfo
	iters::Int32; stop::Int32; n_kl::Int32; j_split::Int32
	Z::Float64; grad_norm::Float64
	ms_rep::Float32; ms_att::Float32; ms_upd::Float32; reserved::Float32
	TmvbMapInfo() = new(0, 0, 0, 0, 0.0, 0.0, 0f0, 0f0, 0f0, 0f0)
end

"""
A 2-D map of the documents of `model` (or of `theta`, K x M topic proportions): t-SNE on the `n_neighbors` nearest documents of each document under
`metric` (:hellinger or :cosine), the repulsion computed exactly over all pairs.  n_neighbors defaults to min(64, M - 1), perplexity to
min(20, n_neighbors / 3).  init = nothing starts from the seeded random state on the device, an M x 2 matrix from that state.  Returns xy (M x 2),
kl and kl_iters (the KL divergence after that many iterations; every `check` iterations and at the end), beta (the precisions of the entropy
search) and the device times.
"""
function map_docs(model::TopicModel; perplexity=nothing, metric::Symbol=:hellinger, n_neighbors=nothing, iters::Integer=750, init=nothing, seed::Integer=0,
				theta=nothing, check::Integer=50, eta=nothing, exaggeration::Real=12.0, exag_iters::Integer=250, device::Integer=0)
	(metric == :hellinger || metric == :cosine)	|| throw(ArgumentError("metric must be :hellinger or :cosine."))
	x = Matrix{Float64}(theta === nothing ? topic_proportions(model) : theta)
	K, M = size(x)
	(M >= 3)							|| throw(TopicModelError("a map needs at least 3 documents."))
	n = n_neighbors === nothing ? min(64, M - 1) : Int(n_neighbors)
	(2 <= n <= min(64, M - 1))			|| throw(ArgumentError("n_neighbors must be an integer in [2, min(64, M - 1)]."))
	u = perplexity === nothing ? min(20.0, n / 3) : Float64(perplexity)
	(1.0 <= u < n)						|| throw(ArgumentError("perplexity must lie in [1, n_neighbors)."))
	(0 <= iters <= 100000 && check >= 0)	|| throw(ArgumentError("iters must lie in [0, 100000] and check must not be negative."))
	y0 = init === nothing ? zeros(Float32, 0, 0) : Matrix{Float32}(permutedims(Matrix{Float32}(init)))		# 2 x M column-major = C's [M][2]
	(init === nothing || size(y0) == (2, M))	|| throw(TopicModelError("init must be an M x 2 matrix."))
	idx = zeros(Int32, n, M); score = zeros(Float32, n, M); count = zeros(Int32, M)		# column-major (j, q) = C's [q][j]
	beta = zeros(Float64, M); pcond = zeros(Float64, n, M)
	row_ptr = zeros(Int64, M + 1); col = zeros(Int32, 2 * M * n); val = zeros(Float32, 2 * M * n)
	y = zeros(Float32, 2, M); vel = zeros(Float32, 2, M); gain = zeros(Float32, 2, M)
	cap = (check > 0 ? div(iters, check) : 0) + 2
	kl = zeros(Float64, cap); kl_iter = zeros(Int32, cap)
	params = TmvbMapParams(iters, 0, exag_iters, check, 0, 0, seed, exaggeration, 0.0, 0.5f0, 0.8f0,
						Float32(eta === nothing ? max(M / exaggeration / 4, 50.0) : eta), 0.01f0)
	info = TmvbMapInfo()
	ctx = tmvb_context(device)
	GC.@preserve x idx score count beta pcond row_ptr col val y0 y vel gain kl kl_iter params info begin
		rc = ccall((:tmvb_topic_neighbors, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64, Int32, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
			ctx, K, NB_METRICS[metric], M, x, M, Ptr{Float64}(C_NULL), 0, n, 0, idx, score, count, C_NULL)
		rc == 0 || tmvb_destroy_context(ctx)
		tmvb_check(rc)
		d2 = map(s -> isfinite(s) ? max(0f0, 2f0 - 2f0 * s) : 0f0, score)
		idx .= max.(idx, Int32(0))
		rc = ccall((:tmvb_map_affinity, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int64, Int64, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}),
			ctx, M, M, n, idx, d2, count, u, beta, pcond, row_ptr, col, val)
		rc == 0 || tmvb_destroy_context(ctx)
		tmvb_check(rc)
		rc = ccall((:tmvb_map_layout, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float32}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
			 Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float32}, Ptr{Cvoid}),
			ctx, M, row_ptr, col, val, pointer_from_objref(params), init === nothing ? Ptr{Float32}(C_NULL) : pointer(y0), Ptr{Float32}(C_NULL), Ptr{Float32}(C_NULL),
			y, vel, gain, cap, kl, kl_iter, Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL), Ptr{Float32}(C_NULL), pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (xy=permutedims(y), kl=kl[1:info.n_kl], kl_iters=Int.(kl_iter[1:info.n_kl]), beta=beta, iters=Int(info.iters), stop=Int(info.stop),
			ms=(repulsion=info.ms_rep, attraction=info.ms_att, update=info.ms_upd))
end

# ---------------------------------------------------------------------------------------------- search documents by words
# Which documents are about these words: tmvb_topic_search scores every query -- sum_j c_j log(theta_d . beta'_{w_j}), the query likelihood of
# LDA-based retrieval -- against every document of the model on the device (probabilities on the f32 MFMA, logarithm and sum in fp64) and keeps,
# per query, the topn best under the total order (score descending, index ascending); neither the probability matrix nor the score matrix exists.

"tmvb_search_info_t (include/tmvb.h), field for field."
mutable struct TmvbSearchInfo
	splits::Int32; kp::Int32; col_tiles::Int32
	ms_prep::Float32; ms_scan::Float32; ms_merge::Float32
	TmvbSearchInfo() = new(0, 0, 0, 0f0, 0f0, 0f0)
end

"One query as (term keys, counts): words through the corpus vocabulary, integers as keys, a Dict as key / word => count; repeated terms are merged."
function search_query(model::TopicModel, q, skip_unknown::Bool)
	keys_of = Dict(name => key for (key, name) in model.corp.vocab)
	terms = Int[]; counts = Int[]
	for (t, c) in (q isa AbstractDict ? collect(q) : [(t, 1) for t in q])
		key = t isa AbstractString ? get(keys_of, t, 0) : Int(t)
		if t isa AbstractString && key == 0
			skip_unknown && continue
			throw(ArgumentError("word \"$t\" is not in the model's vocabulary."))
		end
		(1 <= key <= model.V)			|| throw(ArgumentError("term id $key outside [1, $(model.V)]."))
		(c >= 1)						|| throw(ArgumentError("the count of a term must be a positive integer."))
		i = findfirst(==(key), terms)
		i === nothing ? (push!(terms, key); push!(counts, Int(c))) : (counts[i] += Int(c))
	end
	isempty(terms)						&& throw(ArgumentError("a query is empty."))
	(length(terms) <= 128)				|| throw(ArgumentError("a query has more than 128 distinct terms."))
	return terms, counts
end

"""
(idx, score, count, loglik_per_token) of the `topn` documents under which each query's words are most likely.  `queries` is a vector; each
query is a vector of vocabulary strings, a vector of term keys, or a Dict term => count.  Theta is topic_proportions(model) unless `theta`
(K x M, e.g. of predicted documents) is given.  idx[j, q] is 1-based, 0 past count[q].
"""
function search(model::TopicModel, queries::AbstractVector; topn::Integer=10, laplace_smooth::Real=0.0, theta=nothing, skip_unknown::Bool=false, device::Integer=0)
	model isa hipCTPF					&& throw(TopicModelError("search has no method for CTPF models."))
	(1 <= topn <= 64)					|| throw(ArgumentError("topn must be an integer in [1, 64]."))
	(laplace_smooth >= 0)				|| throw(ArgumentError("laplace_smooth parameter must be nonnegative."))
	isempty(queries)					&& throw(ArgumentError("queries is empty."))
	th = Matrix{Float64}(theta === nothing ? topic_proportions(model) : theta)
	K, Md = size(th)
	beta = Matrix{Float64}(model.beta)
	(size(beta, 1) == K)				|| throw(TopicModelError("theta and model must have the same number of topics."))
	V = size(beta, 2)
	q_ptr = Int64[0]; q_terms = Int32[]; q_counts = Int32[]
	for q in queries
		terms, counts = search_query(model, q, skip_unknown)
		append!(q_terms, Int32.(terms .- 1)); append!(q_counts, Int32.(counts)); push!(q_ptr, length(q_terms))
	end
	Q = length(queries)
	idx = zeros(Int32, topn, Q); score = zeros(Float32, topn, Q); count = zeros(Int32, Q)	# column-major (j, q) = C's [q][j]
	info = TmvbSearchInfo()
	ctx = tmvb_context(device)
	GC.@preserve info th beta q_ptr q_terms q_counts idx score count begin
		rc = ccall((:tmvb_topic_search, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
			ctx, K, V, Md, th, beta, Float64(laplace_smooth), Q, q_ptr, q_terms, q_counts,
			topn, 0, idx, score, count, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	tokens = [sum(q_counts[q_ptr[q]+1:q_ptr[q+1]]) for q in 1:Q]
	return (idx=Int.(idx) .+ 1, score=score, count=Int.(count), loglik_per_token=Float64.(score) ./ reshape(Float64.(tokens), 1, Q),
			info=(splits=Int(info.splits), kp=Int(info.kp), col_tiles=Int(info.col_tiles), ms=(prep=info.ms_prep, scan=info.ms_scan, merge=info.ms_merge)))
end

# ---------------------------------------------------------------------------------------------- word-topic assignments
# Which topic a word belongs to in a document: phi of update_phi! (src/LDA.jl:150-154, src/CTM.jl:175-178, src/CTPF.jl:327-330), which update_host!
# fills in the reference (src/modelutils.jl:514-515, :534-535, :559-560) and the engine never keeps.  tmvb_token_topics recomputes it on the device
# from two nonnegative factors, r_k = (EPSILON + A[k, d] B[k, w]) / sum_j (...), selects the `top` best topics per entry in registers and returns
# dense phi only for the documents asked for.

"tmvb_token_topics_info_t (include/tmvb.h), field for field."
mutable struct TmvbTokenTopicsInfo
	nsel::Int64; n_short::Int64; n_long::Int64
	chunks::Int32; lanes_per_entry::Int32
	ms_kernel::Float32
	TmvbTokenTopicsInfo() = new(0, 0, 0, 0, 0, 0f0)
end

"psi in fp64 by the library's host digamma (tmvb_digamma_f64; touches no device)."
function tmvb_digamma(x::Array{Float64})
	y = similar(x)
	GC.@preserve x y begin
		tmvb_check(ccall((:tmvb_digamma_f64, LIBTMVB), Cint, (Ptr{Float64}, Ptr{Float64}, Int64), x, y, length(x)))
	end
	return y
end

"(A, B), K x M and K x V: the factors of update_phi! by family; the column shifts are taken in fp64 and cancel in the normalisation."
token_factors(model::hipLDA) = (exp.(hcat(model.Elogtheta...)), Matrix{Float64}(model.beta))
function token_factors(model::hipCTM)
	lam = hcat(model.lambda...)
	return exp.(lam .- maximum(lam, dims=1)), Matrix{Float64}(model.beta)
end
function token_factors(model::hipCTPF)
	a = tmvb_digamma(hcat(model.gimel...)) .- log.(model.dalet) .- log.(model.bet)
	b = tmvb_digamma(Matrix{Float64}(model.alef))
	return exp.(a .- maximum(a, dims=1)), exp.(b .- maximum(b, dims=1))
end

function token_topics_call(model::Union{hipLDA, hipCTM, hipCTPF}, docs::Vector{Int}, top::Integer, want_top::Bool, want_phi::Bool, want_hard::Bool, device::Integer)
	(1 <= top <= 8)						|| throw(ArgumentError("top must be an integer in [1, 8]."))
	all(d -> 1 <= d <= model.M, docs)	|| throw(CorpusError("document index outside corpus range."))
	update_host!(model)
	A, B = token_factors(model)
	K, M = size(A); V = size(B, 2)
	doc_ptr, terms, counts = corp_csr(model.corp)
	zdocs = Int32.(docs .- 1)
	Ms = length(zdocs)
	sel_ptr = cumsum(vcat(0, [doc_ptr[d+1] - doc_ptr[d] for d in docs]))
	nsel = sel_ptr[end]
	top_idx = fill(Int32(-1), top, max(nsel, 1)); top_r = zeros(Float32, top, max(nsel, 1))		# column-major (j, n) = C's [n][j]
	phi = zeros(Float32, K, want_phi ? max(nsel, 1) : 1)										# column-major (k, n) = C's [n][k]: the reference's hcat layout
	hard = zeros(Int64, K, max(Ms, 1))
	info = TmvbTokenTopicsInfo()
	ctx = tmvb_context(device)
	GC.@preserve info A B doc_ptr terms counts zdocs top_idx top_r phi hard begin
		rc = ccall((:tmvb_token_topics, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int64, Float64, Int32, Int64, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int64}, Ptr{Cvoid}),
			ctx, K, V, M, A, B, doc_ptr, terms, counts, zdocs, Ms, EPSILON, top, 0,
			want_top ? pointer(top_idx) : Ptr{Int32}(C_NULL), want_top ? pointer(top_r) : Ptr{Float32}(C_NULL), want_phi ? pointer(phi) : Ptr{Float32}(C_NULL), want_hard ? pointer(hard) : Ptr{Int64}(C_NULL), pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (sel_ptr=sel_ptr, nsel=nsel, top_idx=top_idx[:, 1:nsel], top_r=top_r[:, 1:nsel], phi=phi, hard=hard[:, 1:Ms],
			info=(nsel=Int(info.nsel), n_short=Int(info.n_short), n_long=Int(info.n_long), chunks=Int(info.chunks), lanes_per_entry=Int(info.lanes_per_entry), ms_kernel=info.ms_kernel))
end

"""
(topic, prob, hard, doc_ptr, docs) for the entries of the documents `docs` (1-based, repeats allowed; by default every document): topic[j, n] is the
j-th best topic (1-based; 0 past K) of the n-th selected entry, prob[j, n] its responsibility, hard[k, s] the tokens of docs[s] whose best topic is k;
the entries of docs[s] are doc_ptr[s]+1 : doc_ptr[s+1].
"""
function token_topics(model::Union{hipLDA, hipCTM, hipCTPF}; docs=1:0, top::Integer=1, device::Integer=0)
	ds = isempty(docs) ? collect(1:model.M) : collect(Int, docs)
	r = token_topics_call(model, ds, top, true, false, true, device)
	return (topic=Int.(r.top_idx) .+ 1, prob=r.top_r, hard=r.hard, doc_ptr=r.sel_ptr, docs=ds, info=r.info)
end

"phi of document d as the reference keeps it in model.phi (K x N_d, Float32): update_phi! on the device."
function phi(model::Union{hipLDA, hipCTM, hipCTPF}, d::Integer)
	r = token_topics_call(model, [Int(d)], 1, false, true, false, 0)
	return r.phi[:, 1:r.nsel]
end

# ---- held-out recommendation metrics for CTPF (include/tmvb.h: tmvb_readers_split, tmvb_score_ranks, tmvb_rank_metrics) -------------------
# Hold out part of the (document, reader) entries, train on the rest, ask where each held-out document lands in its user's ranking.  The rank of
# a held-out pair is a count -- how many candidates come before it under reverse(sortperm(.)) -- taken in the epilogue of the f32-MFMA score GEMM
# on the device; the split and the metrics are host code of the library.

"tmvb_rsplit_t (include/tmvb.h), field for field."
mutable struct TmvbReaderSplit
	M::Int64; n_obs::Int64; n_held::Int64
	obs_ptr::Ptr{Int64}; obs_readers::Ptr{Int32}; obs_ratings::Ptr{Int32}
	held_ptr::Ptr{Int64}; held_readers::Ptr{Int32}; held_ratings::Ptr{Int32}
	TmvbReaderSplit() = new(0, 0, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL)
end

"tmvb_recranks_info_t (include/tmvb.h), field for field."
mutable struct TmvbRecRanksInfo
	splits::Int32; kp::Int32
	ms_prep::Float32; ms_pairs::Float32; ms_scan::Float32; ms_fix::Float32
	TmvbRecRanksInfo() = new(0, 0, 0f0, 0f0, 0f0, 0f0)
end

const RSPLIT_MODES = Dict(:entry => 0, :document => 1)

"""
(obs, held): the reader CSR (rdr_ptr 0-based offsets, readers 0-based, ratings) split into an observed and a held-out CSR over the same documents,
each a named tuple (ptr, readers, ratings).  mode = :entry holds every entry out with probability frac, :document every document with all of its
readers.  The same seed gives the same split; doc_offset reproduces a slice of a larger call.
"""
function split_readers(rdr_ptr::Vector{Int64}, readers::Vector{Int32}, ratings::Vector{Int32}, U::Integer; frac::Real=0.2, seed::Integer=0,
		doc_offset::Integer=0, mode::Symbol=:entry)
	haskey(RSPLIT_MODES, mode)			|| throw(ArgumentError("mode must be :entry or :document."))
	M = length(rdr_ptr) - 1
	out = TmvbReaderSplit()
	GC.@preserve out rdr_ptr readers ratings begin
		rc = ccall((:tmvb_readers_split, LIBTMVB), Cint,
			(Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Float64, Int64, Int64, Int32, Ptr{Cvoid}),
			M, U, rdr_ptr, readers, ratings, frac, seed, doc_offset, RSPLIT_MODES[mode], pointer_from_objref(out))
		tmvb_check(rc)
		side(p, r, a, n) = (ptr=copy(unsafe_wrap(Array, p, M + 1)), readers=copy(unsafe_wrap(Array, r, n)), ratings=copy(unsafe_wrap(Array, a, n)))
		obs = side(out.obs_ptr, out.obs_readers, out.obs_ratings, out.n_obs)
		held = side(out.held_ptr, out.held_readers, out.held_ratings, out.n_held)
		ccall((:tmvb_rsplit_free, LIBTMVB), Cvoid, (Ptr{Cvoid},), pointer_from_objref(out))
		return obs, held
	end
end

"""
(rank, n_cand, score, ms, splits): for every target id of every query its 0-based rank among the query's candidates (every database row outside
the query's exclusions).  xd: K x Md, xq: K x Mq; excl_ptr / excl_idx and tgt_ptr / tgt_idx: CSR lists of 0-based database ids, strictly
ascending inside a query, the two disjoint.
"""
function score_ranks(xd::Matrix{Float64}, xq::Matrix{Float64}, excl_ptr::Vector{Int64}, excl_idx::Vector{Int32}, tgt_ptr::Vector{Int64},
		tgt_idx::Vector{Int32}; splits::Integer=0, device::Integer=0)
	K, Md = size(xd); Mq = size(xq, 2)
	nT = Int(tgt_ptr[end])
	rank = zeros(Int32, max(nT, 1)); score = zeros(Float32, max(nT, 1)); n_cand = zeros(Int32, Mq)
	info = TmvbRecRanksInfo()
	ctx = tmvb_context(device)
	GC.@preserve info xd xq excl_ptr excl_idx tgt_ptr tgt_idx rank score n_cand begin
		rc = ccall((:tmvb_score_ranks, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Cvoid}),
			ctx, K, Md, xd, Mq, xq, excl_ptr, excl_idx, tgt_ptr, tgt_idx, splits, rank, n_cand, score, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (rank=Int.(rank[1:nT]), n_cand=Int.(n_cand), score=score[1:nT],
			ms=(prep=info.ms_prep, pairs=info.ms_pairs, scan=info.ms_scan, fix=info.ms_fix), splits=Int(info.splits))
end

"tmvb_rectopn_info_t (include/tmvb.h), field for field."
mutable struct TmvbRecTopNInfo
	splits::Int32; kp::Int32
	ms_prep::Float32; ms_scan::Float32; ms_merge::Float32
	TmvbRecTopNInfo() = new(0, 0, 0f0, 0f0, 0f0)
end

"""
(idx, score, count, ms, splits): for every query the `topn` best database rows outside its exclusion list under reverse(sortperm(.)) -- the
head of urecs / drecs without the full ranking.  xd: K x Md, xq: K x Mq; excl_ptr / excl_idx: CSR lists of 0-based database ids, strictly
ascending inside a query.  idx[j, q] is 1-based, 0 past count[q].
"""
function score_topn(xd::Matrix{Float64}, xq::Matrix{Float64}, excl_ptr::Vector{Int64}, excl_idx::Vector{Int32}; topn::Integer=15, splits::Integer=0,
		device::Integer=0)
	(1 <= topn <= 64)					|| throw(ArgumentError("topn must be an integer in [1, 64]."))
	K, Md = size(xd); Mq = size(xq, 2)
	idx = zeros(Int32, topn, Mq); score = zeros(Float32, topn, Mq); count = zeros(Int32, Mq)	# column-major (j, q) = C's [q][j]
	info = TmvbRecTopNInfo()
	ctx = tmvb_context(device)
	GC.@preserve info xd xq excl_ptr excl_idx idx score count begin
		rc = ccall((:tmvb_score_topn, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Int32, Int32, Ptr{Int32}, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
			ctx, K, Md, xd, Mq, xq, excl_ptr, excl_idx, topn, splits, idx, score, count, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (idx=Int.(idx) .+ 1, score=score, count=Int.(count), ms=(prep=info.ms_prep, scan=info.ms_scan, merge=info.ms_merge), splits=Int(info.splits))
end

"tmvb_foldin_info_t (include/tmvb.h), field for field."
mutable struct TmvbFoldinInfo
	kp::Int32; capacity::Int32
	n_reg::Int64; n_long::Int64
	ms_prep::Float32; ms_sweeps::Float32
	TmvbFoldinInfo() = new(0, 0, 0, 0, 0f0, 0f0)
end

"""
(he, sweeps, info): he[:, u] of users who were not in training, iterated with every document factor frozen (include/tmvb.h, "CTPF fold-in").
gimel, zayin: K x M; lib_ptr / lib_docs / lib_ratings: the libraries in CSR form, document ids 0-based and strictly ascending inside a user;
he0: K x Un, or nothing for all ones.
"""
function ctpf_foldin_users(gimel::Matrix{Float64}, zayin::Matrix{Float64}, dalet::Vector{Float64}, het::Vector{Float64}, vav::Vector{Float64}, e::Float64,
		lib_ptr::Vector{Int64}, lib_docs::Vector{Int32}, lib_ratings::Vector{Int32}; he0::Union{Matrix{Float64}, Nothing}=nothing, viter::Integer=10,
		vtol::Real=1/size(gimel, 1)^2, device::Integer=0)
	K, M = size(gimel); Un = length(lib_ptr) - 1
	he = zeros(Float64, K, max(Un, 1)); sweeps = zeros(Int32, max(Un, 1))
	h0 = he0 === nothing ? Ptr{Float64}(C_NULL) : pointer(he0)
	info = TmvbFoldinInfo()
	ctx = tmvb_context(device)
	GC.@preserve info gimel zayin dalet het vav lib_ptr lib_docs lib_ratings he0 he sweeps begin
		rc = ccall((:tmvb_ctpf_foldin_users, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}),
			ctx, K, M, gimel, zayin, dalet, het, vav, e, Un, lib_ptr, lib_docs, lib_ratings, h0, viter, vtol, he, sweeps, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (he=he[:, 1:Un], sweeps=Int.(sweeps[1:Un]), info=info)
end

"The same on the device-resident state of a CTPF handle (`handle`: the Ptr{Cvoid} of tmvb_ctpf_create): no K x M upload."
function ctpf_foldin_users_on(handle::Ptr{Cvoid}, K::Integer, lib_ptr::Vector{Int64}, lib_docs::Vector{Int32}, lib_ratings::Vector{Int32};
		he0::Union{Matrix{Float64}, Nothing}=nothing, viter::Integer=10, vtol::Real=1/K^2)
	Un = length(lib_ptr) - 1
	he = zeros(Float64, K, max(Un, 1)); sweeps = zeros(Int32, max(Un, 1))
	h0 = he0 === nothing ? Ptr{Float64}(C_NULL) : pointer(he0)
	info = TmvbFoldinInfo()
	GC.@preserve info lib_ptr lib_docs lib_ratings he0 he sweeps begin
		rc = ccall((:tmvb_ctpf_foldin_users_on, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}, Int32, Float64, Ptr{Float64}, Ptr{Int32}, Ptr{Cvoid}),
			handle, Un, lib_ptr, lib_docs, lib_ratings, h0, viter, vtol, he, sweeps, pointer_from_objref(info))
		tmvb_check(rc)
	end
	return (he=he[:, 1:Un], sweeps=Int.(sweeps[1:Un]), info=info)
end

"""
recall / precision / ndcg (length(topn) x Mq), mrr, pct_rank (Mq; NaN for a query without targets), their means over the queries with targets
(recall@topn, precision@topn, ndcg@topn, mrr, pct_rank, in that order), the number of such queries and the number of targets.
"""
function rank_metrics(tgt_ptr::Vector{Int64}, rank::Vector{Int32}, n_cand::Vector{Int32}; topn::Vector{Int32}=Int32[10, 20, 50, 100])
	Mq = length(tgt_ptr) - 1; nN = length(topn)
	recall = zeros(Float64, nN, Mq); precision = zeros(Float64, nN, Mq); ndcg = zeros(Float64, nN, Mq)		# column-major (a, q) = C's [q][a]
	mrr = zeros(Float64, Mq); pct_rank = zeros(Float64, Mq); means = zeros(Float64, 3nN + 2); counts = zeros(Int64, 2)
	rc = ccall((:tmvb_rank_metrics, LIBTMVB), Cint,
		(Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}),
		Mq, tgt_ptr, rank, n_cand, nN, topn, recall, precision, ndcg, mrr, pct_rank, means, counts)
	tmvb_check(rc)
	return (recall=recall, precision=precision, ndcg=ndcg, mrr=mrr, pct_rank=pct_rank, means=means, n_queries=Int(counts[1]), n_targets=Int(counts[2]))
end

# ---------------------------------------------------------------------------------------------- compare topics
# The topic side of a model: tmvb_topic_divergence (pairwise Jensen-Shannon / Hellinger / total variation / KL between the rows of one or two K x V
# topic-word matrices, fp64, every sum in one fixed order), tmvb_assignment (minimum-cost matching of the topics of two runs, host only) and
# tmvb_term_relevance (the relevance ranking of LDAvis with distinctiveness and saliency).  include/tmvb.h is the specification.

"tmvb_topicdiv_info_t (include/tmvb.h), field for field."
mutable struct TmvbTopicDivInfo
	splits::Int32; runs::Int32
	ms_prep::Float32; ms_pairs::Float32; ms_merge::Float32
	TmvbTopicDivInfo() = new(0, 0, 0f0, 0f0, 0f0)
end

"tmvb_relevance_info_t (include/tmvb.h), field for field."
mutable struct TmvbRelevanceInfo
	ms_score::Float32; ms_select::Float32; ms_terms::Float32
	TmvbRelevanceInfo() = new(0f0, 0f0, 0f0)
end

const TD_METRICS = Dict(:js => 0, :hellinger => 1, :tv => 2, :kl => 3)

"""
D[i, j] = the divergence of row i of `a` (KA x V, rows are distributions: model.beta) from row j of `b` (KB x V; nothing: of `a` itself).
metric :js (nats), :hellinger, :tv or :kl (directed; smooth > 0 keeps it finite).
"""
function topic_divergence(a::Matrix{Float64}, b::Union{Nothing, Matrix{Float64}}=nothing; metric::Symbol=:js, smooth::Real=0.0, splits::Integer=0,
						  device::Integer=0)
	haskey(TD_METRICS, metric)			|| throw(ArgumentError("metric must be :js, :hellinger, :tv or :kl."))
	KA, V = size(a)
	KB = b === nothing ? KA : size(b, 1)
	(b === nothing || size(b, 2) == V)	|| throw(TopicModelError("a and b must be over the same vocabulary."))
	Dt = zeros(Float64, KB, KA)			# C's row-major [KA][KB]
	info = TmvbTopicDivInfo()
	ctx = tmvb_context(device)
	GC.@preserve info a b Dt begin
		rc = ccall((:tmvb_topic_divergence, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Int32, Ptr{Float64}, Int32, Ptr{Float64}, Float64, Int32, Ptr{Float64}, Ptr{Cvoid}),
			ctx, TD_METRICS[metric], V, KA, a, KB, b === nothing ? Ptr{Float64}(C_NULL) : pointer(b), smooth, splits, Dt, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (distance=permutedims(Dt), splits=Int(info.splits), runs=Int(info.runs), ms=(prep=info.ms_prep, pairs=info.ms_pairs, merge=info.ms_merge))
end

"""
A minimum-cost assignment of the n rows of `cost` (n x m, n <= m, entries finite or Inf) to distinct columns: (match, total), match[i] 1-based.
"""
function assignment(cost::Matrix{Float64})
	n, m = size(cost)
	ct = permutedims(cost)				# C's row-major [n][m]
	match = zeros(Int32, n); total = zeros(Float64, 1)
	rc = ccall((:tmvb_assignment, LIBTMVB), Cint, (Int32, Int32, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}), n, m, ct, match, total)
	tmvb_check(rc)
	return (match=Int.(match) .+ 1, total=total[1])
end

"""
The `topn` terms of every topic by relevance lambda log(phi) + (1 - lambda) log(phi / pw), 1-based (0 past count), with their scores, and the
distinctiveness and saliency of every term.  beta K x V, pw[V] the marginal term probabilities, pi[K] the topic shares.
"""
function term_relevance(beta::Matrix{Float64}, pw::Vector{Float64}, pi::Vector{Float64}; lambda::Real=0.6, topn::Integer=10, device::Integer=0)
	K, V = size(beta)
	(length(pw) == V && length(pi) == K)	|| throw(TopicModelError("pw must have V entries and pi K."))
	idx = zeros(Int32, topn, K); score = zeros(Float64, topn, K); count = zeros(Int32, K)		# column-major (slot, k) = C's [k][slot]
	distinct = zeros(Float64, V); saliency = zeros(Float64, V)
	info = TmvbRelevanceInfo()
	ctx = tmvb_context(device)
	GC.@preserve info beta pw pi idx score count distinct saliency begin
		rc = ccall((:tmvb_term_relevance, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Int32, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64},
			 Ptr{Float64}, Ptr{Cvoid}),
			ctx, K, V, beta, pw, pi, lambda, topn, idx, score, count, Ptr{Float64}(C_NULL), distinct, saliency, pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (idx=permutedims(Int.(idx) .+ 1), score=permutedims(score), count=Int.(count), distinctiveness=distinct, saliency=saliency,
			ms=(score=info.ms_score, select=info.ms_select, terms=info.ms_terms))
end

# ---- topics by group and over time (include/tmvb.h: tmvb_group_topics, tmvb_group_index) ---------------------------------------------------
# For every group g of documents S_g[k, w] = the sum over the entries (w, c) of the documents of g of c r_k(d, w), r the responsibilities of
# tmvb_token_topics; from it the topic masses, the top words of every topic inside the group, its Jensen-Shannon shift from the pooled topic and
# its drift from the previous group.  include/tmvb.h is the specification.

"tmvb_group_topics_info_t (include/tmvb.h), field for field."
mutable struct TmvbGroupTopicsInfo
	nsel::Int64; runs::Int64; segments::Int64
	group_chunks::Int32; lanes_per_entry::Int32
	ms_index::Float32; ms_accum::Float32; ms_select::Float32; ms_shift::Float32
	TmvbGroupTopicsInfo() = new(0, 0, 0, 0, 0, 0f0, 0f0, 0f0, 0f0)
end

"""
Topics by group: `group[d]` in 1:G names the group of document d of the model's corpus, 0 leaves the document out.  Returns docs[G], tokens[G],
mass[K, G], prevalence[K, G], idx[topn, K, G] (1-based term ids, 0 for a group without entries), prob[topn, K, G], shift[K, G] and drift[K, G].
"""
function group_topics(model::Union{hipLDA, hipCTM, hipCTPF}, group::Vector{<:Integer}, G::Integer; topn::Integer=10, device::Integer=0)
	length(group) == model.M			|| throw(ArgumentError("group must hold one label per document."))
	all(g -> 0 <= g <= G, group)		|| throw(ArgumentError("group labels must lie in 0:G."))
	update_host!(model)
	A, B = token_factors(model)
	K, M = size(A); V = size(B, 2)
	doc_ptr, terms, counts = corp_csr(model.corp)
	zgroup = Int32.(group .- 1)
	docs = zeros(Int64, G); tokens = zeros(Int64, G)
	mass = zeros(Float64, K, G)										# column-major (k, g) = C's [g][k]
	idx = fill(Int32(-1), topn, K, G); prob = zeros(Float64, topn, K, G)
	shift = zeros(Float64, K, G); drift = zeros(Float64, K, G)
	info = TmvbGroupTopicsInfo()
	ctx = tmvb_context(device)
	GC.@preserve info A B doc_ptr terms counts zgroup docs tokens mass idx prob shift drift begin
		rc = ccall((:tmvb_group_topics, LIBTMVB), Cint,
			(Ptr{Cvoid}, Int32, Int64, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Float64, Int32, Int32,
			 Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cvoid}),
			ctx, K, V, M, A, B, doc_ptr, terms, counts, zgroup, G, EPSILON, topn, 0,
			docs, tokens, mass, idx, prob, shift, drift, Ptr{Float64}(C_NULL), pointer_from_objref(info))
		tmvb_destroy_context(ctx)
		tmvb_check(rc)
	end
	return (docs=docs, tokens=tokens, mass=mass, prevalence=mass ./ sum(mass, dims=1), idx=Int.(idx) .+ 1, prob=prob, shift=shift, drift=drift,
			info=(nsel=Int(info.nsel), runs=Int(info.runs), segments=Int(info.segments), group_chunks=Int(info.group_chunks),
				  lanes_per_entry=Int(info.lanes_per_entry), ms_index=info.ms_index, ms_accum=info.ms_accum, ms_select=info.ms_select, ms_shift=info.ms_shift))
end

"The (group, term) index tmvb_group_topics walks (host only): (run_ptr, run_group, run_term, entry), 0-based as the library returns them."
function group_index(doc_ptr::Vector{Int64}, terms::Vector{Int32}, group::Vector{Int32}, G::Integer, V::Integer)
	M = length(doc_ptr) - 1
	nsel = sum(Int[doc_ptr[d+1] - doc_ptr[d] for d in 1:M if group[d] >= 0])
	n_runs = Ref{Int64}(0)
	run_ptr = zeros(Int64, nsel + 1); run_group = zeros(Int32, max(nsel, 1)); run_term = zeros(Int32, max(nsel, 1)); entry = zeros(Int64, max(nsel, 1))
	rc = ccall((:tmvb_group_index, LIBTMVB), Cint,
		(Int64, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Ref{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
		M, V, doc_ptr, terms, group, G, n_runs, run_ptr, run_group, run_term, entry)
	tmvb_check(rc)
	r = n_runs[]
	return (run_ptr=run_ptr[1:r+1], run_group=run_group[1:r], run_term=run_term[1:r], entry=entry[1:nsel])
end
