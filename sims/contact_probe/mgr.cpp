#include "contact_probe/sim.hpp"

#include <madrona/physics_loader.hpp>
#include <madrona/physics_assets.hpp>
#include <madrona/importer.hpp>
#include <madrona/stack_alloc.hpp>

struct SimTraits;
#include "common/sim_c_api.h"

#include <array>
#include <vector>
#include <string>
#include <memory>

namespace {

using namespace madrona;
using namespace madrona::phys;
using contactprobe::SimObject;

std::vector<std::unique_ptr<PhysicsLoader>> &loaders()
{
    static std::vector<std::unique_ptr<PhysicsLoader>> list;
    return list;
}

// Cube: the unit-cube hull of escape_room_phys (same vertex and face order);
// Plane; Sphere of radius 0.7
ObjectManager *loadObjects(const SimCreateArgs &args)
{
#ifdef SIM_BACKEND_REF_CPU
    (void)args;
    auto loader = std::make_unique<PhysicsLoader>(ExecMode::CPU, 4);
#else
    auto loader = std::make_unique<PhysicsLoader>(ExecMode::CUDA, 4, args.gpu_id);
#endif

    math::Vector3 positions[8] = {
        { -0.5f, -0.5f, -0.5f }, { 0.5f, -0.5f, -0.5f },
        { 0.5f, 0.5f, -0.5f }, { -0.5f, 0.5f, -0.5f },
        { -0.5f, -0.5f, 0.5f }, { 0.5f, -0.5f, 0.5f },
        { 0.5f, 0.5f, 0.5f }, { -0.5f, 0.5f, 0.5f },
    };
    uint32_t indices[24] = {
        0, 3, 2, 1,     // -z
        4, 5, 6, 7,     // +z
        0, 1, 5, 4,     // -y
        2, 3, 7, 6,     // +y
        0, 4, 7, 3,     // -x
        1, 2, 6, 5,     // +x
    };
    uint32_t face_counts[6] = { 4, 4, 4, 4, 4, 4 };

    imp::SourceMesh hull_mesh {};
    hull_mesh.positions = positions;
    hull_mesh.indices = indices;
    hull_mesh.faceCounts = face_counts;
    hull_mesh.numVertices = 8;
    hull_mesh.numFaces = 6;

    std::array<SourceCollisionPrimitive, (size_t)SimObject::NumObjects> prims {};
    std::array<SourceCollisionObject, (size_t)SimObject::NumObjects> objs {};

    prims[(size_t)SimObject::Cube].type = CollisionPrimitive::Type::Hull;
    prims[(size_t)SimObject::Cube].hullInput.hullIDX = 0;
    prims[(size_t)SimObject::Plane].type = CollisionPrimitive::Type::Plane;
    prims[(size_t)SimObject::Sphere].type = CollisionPrimitive::Type::Sphere;
    prims[(size_t)SimObject::Sphere].sphere.radius = 0.7f;
    const float inv_mass[(size_t)SimObject::NumObjects] = { 1.f, 0.f, 1.f };
    for (size_t i = 0; i < (size_t)SimObject::NumObjects; i++) {
        objs[i] = SourceCollisionObject {
            Span<const SourceCollisionPrimitive>(&prims[i], 1),
            inv_mass[i], { 0.5f, 0.5f },
        };
    }

    StackAlloc tmp_alloc;
    RigidBodyAssets assets;
    CountT num_bytes;
    void *data = RigidBodyAssets::processRigidBodyAssets(
        Span<const imp::SourceMesh>(&hull_mesh, 1),
        Span<const SourceCollisionObject>(objs.data(), (CountT)objs.size()),
        false, tmp_alloc, &assets, &num_bytes);
    if (data == nullptr) {
        FATAL("Invalid collision hull input");
    }

    loader->loadRigidBodies(assets);
    free(data);

    ObjectManager *mgr = &loader->getObjectManager();
    loaders().push_back(std::move(loader));
    return mgr;
}

}

struct SimTraits {
    using Sim = contactprobe::Sim;
    using Engine = contactprobe::Engine;

    static constexpr uint32_t numExports = (uint32_t)contactprobe::ExportID::NumExports;
    static constexpr uint32_t numTaskGraphs = 1;

    static Sim::Config makeConfig(const SimCreateArgs &args)
    {
        return Sim::Config { args.seed, args.world_base, loadObjects(args) };
    }

    static void makeInits(const SimCreateArgs &, Sim::WorldInit *) {}

    template <typename T>
    static void describeTensors(T &out, uint32_t num_worlds);
    template <typename T>
    static void describeColumns(T &cols);
};

#include "common/mgr_impl.inl"

template <typename T>
void SimTraits::describeTensors(T &out, uint32_t num_worlds)
{
    out.push_back({ "step_count", SIM_I32, { (int64_t)num_worlds, 1 },
                    (uint32_t)contactprobe::ExportID::StepCount });
}

// what the definition of a contact reads (madrona_amd/contact_ref.py)
template <typename T>
void SimTraits::describeColumns(T &cols)
{
    using namespace contactprobe;
    using madrona::Entity;
    using namespace madrona::phys;
    using madrona::base::Scale;
    using madrona::base::ObjectID;

    cols.template add<Body, Entity>("Body.Entity", false);
    cols.template add<Body, Position>("Body.Position", true);
    cols.template add<Body, Rotation>("Body.Rotation", true);
    cols.template add<Body, Scale>("Body.Scale", true);
    cols.template add<Body, ObjectID>("Body.ObjectID", false);
    cols.template add<Body, ResponseType>("Body.ResponseType", false);
    cols.template add<Body, Velocity>("Body.Velocity", true);
#ifndef SIM_BACKEND_REF_CPU
    // the poses the solver's last substep built its contacts at: the reference
    // keeps the component out of its public headers
    cols.template add<Body, xpbd::PreSolvePositional>("Body.PreSolvePositional", true);
#endif
}
